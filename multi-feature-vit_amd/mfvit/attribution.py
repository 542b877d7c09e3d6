"""Gradient attribution for the image encoders and the two-stream model: integrated gradients (Sundararajan, Taly & Yan 2017), SmoothGrad
(Smilkov et al. 2017) and plain saliency (Simonyan et al. 2014) - the gradient baselines that every relevance paper compares its maps with.

    res = integrated_gradients(vit, img, target=y, steps=20)       # res.maps (B, gh, gw) goes straight into perturbation_test
    res = smoothgrad(vit, img, target=y, samples=25, seed=1)
    (rc, re), share = fus.integrated_gradients(vit_cxr, vit_enh, xc, xe, target=y)     # share: how much of the logit came from the CXR stream

Every method is the same loop: build the S inputs of a forward group (mfvit_attr_inputs: path points base + alpha (x - base), optional
counter-hash Gaussian noise), run an evaluation forward with saved activations and the data-gradient-only backward of the target's score
(mfvit_vit_backward_ex with dparams = NULL: no weight gradient, no gradient arena, no p.grad, whatever requires_grad says), add the weighted
image gradients (mfvit_attr_accumulate), and at the end multiply by the input difference, fold the channels, pool 16 x 16 patches and sum
(mfvit_attr_finish).  Integrated gradients are complete: the attributions sum to score(x) - score(baseline) up to the quadrature error, which
`delta` reports; along the joint path of the two-stream model the two streams' totals split that difference between the streams.

Contract of every call: evaluation mode throughout; p.grad, gradient arenas, feature caches, training flags and RNG state (apart from one
drawn seed) stay as they were; no host synchronisation (AttributionResult.cpu() is the one copy); max_batch >= B bounds the images per
forward, steps are forwarded whole; the encoder picks kernels by row count, so results are bit-reproducible for a fixed max_batch, not across
different ones.  Argument errors raise ValueError before any launch, CPU tensors MfvitError.

Limits: one GPU; patch pooling fixed at 16; baselines are constants or a caller-supplied tensor (a blurred image is such a tensor);
first-order only (create_graph stays an error).
"""
import math

import torch

from ._lib import check, lib, ptr, require_cuda, stream
from .encoder import check_target, eval_modules
from .perturb import _as_int as _index, _groups

RULES = ("trapezoid", "midpoint")
SCORES = ("logit", "prob")
SIGNS = ("signed", "abs")
STREAMS = ("both", "cxr", "enh")


# ---------------------------------------------------------------------------------------------------- host-side tables and checks
def _as_int(v, what, lo):
    v = _index(v, what)
    if v < lo:
        raise ValueError(f"{what} must be at least {lo}, got {v}")
    return v


def path_table(steps, rule="trapezoid"):
    """(alphas, weights) of the quadrature of integrated gradients along base + alpha (x - base), as float64 lists: 'trapezoid' uses the
    steps + 1 points i / steps with the end points at half weight, 'midpoint' the steps points (i + 1/2) / steps.  The weights sum to 1."""
    steps = _as_int(steps, "steps", 1)
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
    if rule == "trapezoid":
        return [i / steps for i in range(steps + 1)], [(0.5 if i in (0, steps) else 1.0) / steps for i in range(steps + 1)]
    return [(i + 0.5) / steps for i in range(steps)], [1.0 / steps] * steps


def _check_img(img, what):
    if not isinstance(img, torch.Tensor) or img.dim() != 4:
        raise ValueError(f"{what}: the images must be a (B, C, H, W) tensor")
    B, C, H, W = (int(v) for v in img.shape)
    if B < 1 or C < 1 or H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError(f"{what}: need at least one image with H and W positive multiples of 16, got {tuple(img.shape)}")
    return B, C, H, W


def _check_baseline(baseline, shape):
    """None (zeros), a number, one number per channel, or a full tensor of the image's shape -> (f32 CPU / device tensor or None, full)."""
    B, C, H, W = shape
    if baseline is None:
        return None, False
    if isinstance(baseline, torch.Tensor) and baseline.dim() == 4:
        if tuple(baseline.shape) != shape:
            raise ValueError(f"a baseline tensor must have the images' shape {shape}, got {tuple(baseline.shape)}")
        return baseline, True
    try:
        b = (baseline.detach() if isinstance(baseline, torch.Tensor) else torch.as_tensor(baseline)).to(torch.float32).reshape(-1)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"baseline must be None, a number, {C} numbers or a {shape} tensor, got {baseline!r}") from None
    if b.numel() == 1:
        b = b.expand(C)
    if b.numel() != C:
        raise ValueError(f"baseline must be None, one number, {C} numbers (one per channel) or a {shape} tensor, got {b.numel()} numbers")
    return b, False


def _check_common(score, sign, max_batch, B):
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    if sign not in SIGNS:
        raise ValueError(f"sign must be one of {SIGNS}, got {sign!r}")
    if max_batch is not None and _as_int(max_batch, "max_batch", 1) < B:
        raise ValueError(f"max_batch = {max_batch} is smaller than the batch ({B} images): steps are forwarded whole")


def _check_noise(noise_level, seed):
    try:
        level = float(noise_level)
    except (TypeError, ValueError):
        raise ValueError(f"noise_level must be a number, got {noise_level!r}") from None
    if not level >= 0.0 or math.isinf(level):
        raise ValueError(f"noise_level must be a finite number >= 0, got {noise_level!r}")
    if seed is not None and not 0 <= _as_int(seed, "seed", 0) < 2 ** 63:
        raise ValueError(f"seed must lie in [0, 2^63), got {seed!r}")
    return level


# ---------------------------------------------------------------------------------------------------- thin wrappers of the three launches
def attr_inputs(x, base, alpha, sigma=None, seed=None, s0=0):
    """x f32 (B, C, H, W), base f32 (C,) or (B, C, H, W), alpha device f32 (S,), sigma device f32 (B,) or None, seed device int64 (1,) ->
    f32 (S, B, C, H, W): base + alpha (x - base) (+ sigma z); include/mfvit.h, mfvit_attr_inputs."""
    B, C, H, W = (int(v) for v in x.shape)
    S = int(alpha.shape[0])
    out = torch.empty(S, B, C, H, W, device=x.device, dtype=torch.float32)
    check(lib().mfvit_attr_inputs(ptr(x), ptr(base), int(base.dim() == 4), ptr(alpha), ptr(sigma), ptr(seed), int(s0), ptr(out), S, B, C, H * W,
                                  stream()), "mfvit_attr_inputs")
    return out


def attr_accumulate(g, w, acc, power=1):
    """acc (B, ..) += sum_s w[s] g[s]^power for g f32 (k, B, ..), w device f32 (k,); include/mfvit.h, mfvit_attr_accumulate."""
    k, B = int(g.shape[0]), int(g.shape[1])
    check(lib().mfvit_attr_accumulate(ptr(g), ptr(w), ptr(acc), k, B, acc[0].numel(), int(power), stream()), "mfvit_attr_accumulate")


def attr_finish(acc, x=None, base=None, absval=False, return_pixels=False):
    """acc f32 (B, C, H, W) (times x - base when x is given) -> (maps f32 (B, H/16, W/16), pixels f32 (B, H, W) or None, total f64 (B,));
    include/mfvit.h, mfvit_attr_finish."""
    B, C, H, W = (int(v) for v in acc.shape)
    maps = torch.empty(B, H // 16, W // 16, device=acc.device, dtype=torch.float32)
    pixels = torch.empty(B, H, W, device=acc.device, dtype=torch.float32) if return_pixels else None
    total = torch.empty(B, device=acc.device, dtype=torch.float64)
    check(lib().mfvit_attr_finish(ptr(acc), ptr(x), ptr(base), int(base is not None and base.dim() == 4), int(x is not None), int(bool(absval)),
                                  ptr(pixels), ptr(maps), ptr(total), B, C, H, W, stream()), "mfvit_attr_finish")
    return maps, pixels, total


# ---------------------------------------------------------------------------------------------------- the result
class AttributionResult:
    """maps (B, gh, gw) f32: the attribution summed over every 16 x 16 patch; pixels (B, H, W) f32 or None; total (B,) f64: the sum of the
    SIGNED attribution (also with sign='abs').  Integrated gradients add score_input, score_baseline (B,) f64 and
    delta = total - (score_input - score_baseline), the completeness gap (for the two-stream model: of both streams' totals together).
    Everything lives on the device; cpu() returns a copy on the host and is the single device-to-host transfer."""
    FIELDS = ("maps", "pixels", "total", "score_input", "score_baseline", "delta")

    def __init__(self, maps, pixels, total, score_input=None, score_baseline=None, delta=None):
        self.maps, self.pixels, self.total = maps, pixels, total
        self.score_input, self.score_baseline, self.delta = score_input, score_baseline, delta

    def cpu(self):
        held = [(k, getattr(self, k)) for k in self.FIELDS if getattr(self, k) is not None]
        if not held or not held[0][1].is_cuda:
            return self
        flat = torch.cat([v.detach().double().reshape(-1) for _, v in held]).cpu()      # (f32 -> f64 -> f32 is exact) the one copy
        out, at = {}, 0
        for k, v in held:
            out[k] = flat[at:at + v.numel()].view(v.shape).to(v.dtype)
            at += v.numel()
        return AttributionResult(**{k: out.get(k) for k in self.FIELDS})

    def __repr__(self):
        return "AttributionResult(" + ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.FIELDS if getattr(self, k) is not None) + ")"


# ---------------------------------------------------------------------------------------------------- encoder plumbing
def _eval_features(vit, img):
    """features3D of an evaluation forward without saved activations; the feature cache is left alone."""
    img = vit._prep_img(img.detach())
    with torch.no_grad():
        cfg = vit._cfg(img, False)
        cache = vit._feat_cache
        vit._ensure_shadow(cfg)
        vit._feat_cache = cache
        ws = vit._get_ws(cfg)
        feats = torch.empty(img.shape[0], vit.num_tokens, vit.embed_dim, device=img.device, dtype=torch.float32)
        try:
            check(lib().mfvit_vit_forward(cfg, ptr(vit._kernel_params()), ptr(vit._shadow), ptr(img), ptr(ws), ptr(feats), stream()), "mfvit_vit_forward")
        finally:
            vit._release_ws(ws)
    return feats


def _saved_forward(vit, img):
    """Evaluation forward with saved activations on a workspace that can hold the image gradient: (cfg, workspace, features).  The caller
    releases the workspace."""
    img = vit._prep_img(img.detach())
    with torch.no_grad():
        cfg = vit._cfg(img, True)
        cache = vit._feat_cache
        vit._ensure_shadow(cfg)
        vit._feat_cache = cache
        ws = vit._get_ws(cfg, None, want_dimg=True)
        feats = torch.empty(img.shape[0], vit.num_tokens, vit.embed_dim, device=img.device, dtype=torch.float32)
        try:
            check(lib().mfvit_vit_forward(cfg, ptr(vit._kernel_params()), ptr(vit._shadow), ptr(img), ptr(ws), ptr(feats), stream()), "mfvit_vit_forward")
        except BaseException:
            vit._release_ws(ws)
            raise
    return cfg, ws, feats


def _image_gradient(vit, cfg, ws, dfeats, shape):
    """d score / d img of a _saved_forward by the data-gradient-only backward: no parameter gradient of any stage is formed."""
    dimg = torch.empty(shape, device=dfeats.device, dtype=torch.float32)
    with torch.no_grad():
        vit._run_backward(cfg, ws, dfeats.detach(), dimg=dimg, want_params=False)
    return dimg


def _score_of(out, idx, score):
    """(N, 1) score of the target class: its logit, or its softmax probability (plain torch on the (N, classes) output)."""
    return (out.float().softmax(dim=1) if score == "prob" else out.float()).gather(1, idx)


class _Stream:
    """One image input of a model: the prepared image, its baseline on the device and whether it is attributed (or stays at its input)."""

    def __init__(self, vit, img, baseline, active):
        self.vit, self.active = vit, active
        self.x = vit._prep_img(img.detach())
        C = int(self.x.shape[1])
        b, self.base_full = baseline
        if b is None:
            self.base = torch.zeros(C, dtype=torch.float32, device=self.x.device)
        else:
            self.base = b.detach().to(self.x.device, torch.float32).contiguous()

    def base_image(self):
        return self.base if self.base_full else self.base.view(1, -1, 1, 1).expand_as(self.x).contiguous()


def _single_model(vit):
    """(forward with the image gradient, forward alone) of one encoder and its head."""
    def fwd_bwd(streams, xs, idx, score):
        cfg, ws, feats = _saved_forward(vit, xs[0])
        try:
            f = feats.detach().requires_grad_(True)
            with torch.enable_grad():
                out = vit.forward_head(f)
                (df,) = torch.autograd.grad(_score_of(out, idx, score).sum(), f)
            return out.detach(), [_image_gradient(vit, cfg, ws, df, xs[0].shape)]
        finally:
            vit._release_ws(ws)

    def fwd(streams, xs):
        with torch.no_grad():
            return vit.forward_head(_eval_features(vit, xs[0]))
    return fwd_bwd, fwd


def _two_stream_model(out_of):
    """The same for a two-stream model whose output on the two encoders' features is out_of(f_cxr, f_enh).  An inactive stream runs a plain
    evaluation forward; the encoders run one after the other on the caller's stream."""
    def fwd_bwd(streams, xs, idx, score):
        held = []
        try:
            leaves = []
            for st, x in zip(streams, xs):
                if st.active:
                    cfg, ws, feats = _saved_forward(st.vit, x)
                    held.append((st.vit, ws))
                    leaves.append((feats.detach().requires_grad_(True), cfg, ws))
                else:
                    leaves.append((_eval_features(st.vit, x), None, None))
            with torch.enable_grad():
                out = out_of(leaves[0][0], leaves[1][0])
                dfs = torch.autograd.grad(_score_of(out, idx, score).sum(), [l[0] for l, st in zip(leaves, streams) if st.active])
            dfs, grads = list(dfs), []
            for st, x, (_, cfg, ws) in zip(streams, xs, leaves):
                grads.append(_image_gradient(st.vit, cfg, ws, dfs.pop(0), x.shape) if st.active else None)
            return out.detach(), grads
        finally:
            for vit, ws in held:
                vit._release_ws(ws)

    def fwd(streams, xs):
        with torch.no_grad():
            return out_of(_eval_features(streams[0].vit, xs[0]), _eval_features(streams[1].vit, xs[1]))
    return fwd_bwd, fwd


# ---------------------------------------------------------------------------------------------------- the loop
def _attribute(streams, model, mods, B, tgt, alphas, weights, power, level, seed, times_input, sign, score, max_batch, return_pixels, endpoints):
    """The shared loop.  streams: [_Stream]; model: (fwd_bwd, fwd); tgt: CPU int64 (B,) or None; level: noise level (0: none); endpoints:
    report score_input / score_baseline / delta (integrated gradients).  Returns ([AttributionResult or None per stream], joint total)."""
    fwd_bwd, fwd = model
    dev = streams[0].x.device
    S = len(alphas)
    saved = [(st.vit, st.vit._feat_cache, getattr(st.vit, "_grad_arena_lent", False)) for st in streams]
    try:
        with eval_modules(*mods):
            al, wt = torch.tensor(alphas, dtype=torch.float32).to(dev), torch.tensor(weights, dtype=torch.float32).to(dev)
            sigma, seeds = [None] * len(streams), [None] * len(streams)
            if level > 0.0:
                # one seed per call (drawn on the device: no synchronisation), stream i uses seed + i
                sd = torch.randint(0, 2 ** 62, (1,), device=dev, dtype=torch.int64) if seed is None else torch.tensor([seed], dtype=torch.int64).to(dev)
                for i, st in enumerate(streams):
                    if st.active:
                        sigma[i] = ((st.x.amax(dim=(1, 2, 3)) - st.x.amin(dim=(1, 2, 3))) * level).contiguous()
                        seeds[i] = sd + i
            if tgt is None:
                idx = fwd(streams, [st.x for st in streams]).argmax(dim=1, keepdim=True)
            else:
                idx = tgt.to(dev).view(-1, 1)
            acc = [torch.zeros_like(st.x) if st.active else None for st in streams]
            scores = torch.empty(S, B, device=dev, dtype=torch.float64)
            for s0, s1 in _groups(S, B, max_batch):
                k = s1 - s0
                xs = [attr_inputs(st.x, st.base, al[s0:s1], sigma[i], seeds[i], s0).flatten(0, 1) if st.active
                      else (st.x if k == 1 else st.x.repeat(k, 1, 1, 1)) for i, st in enumerate(streams)]
                out, grads = fwd_bwd(streams, xs, idx if k == 1 else idx.repeat(k, 1), score)
                if tgt is not None and tgt.numel() and int(tgt.max()) >= out.shape[1]:
                    raise ValueError(f"target class out of range for {out.shape[1]} classes: {tgt.tolist()}")
                with torch.no_grad():
                    scores[s0:s1] = _score_of(out, idx if k == 1 else idx.repeat(k, 1), score).view(k, B)
                    for a, g in zip(acc, grads):
                        if a is not None:
                            attr_accumulate(g.view(k, *a.shape), wt[s0:s1], a, power)
            with torch.no_grad():
                s_in = s_base = None
                if endpoints:
                    if level == 0.0 and alphas[0] == 0.0 and alphas[-1] == 1.0:
                        s_base, s_in = scores[0], scores[-1]                 # the path's own end points
                    else:
                        s_in = _score_of(fwd(streams, [st.x for st in streams]), idx, score).view(B).double()
                        s_base = _score_of(fwd(streams, [st.base_image() if st.active else st.x for st in streams]), idx, score).view(B).double()
                fin = [attr_finish(a, st.x if times_input else None, st.base if times_input else None, sign == "abs", return_pixels)
                       if a is not None else None for a, st in zip(acc, streams)]
                joint = sum(f[2] for f in fin if f is not None)
                delta = joint - (s_in - s_base) if endpoints else None
                return [None if f is None else AttributionResult(f[0], f[1], f[2], s_in, s_base, delta) for f in fin], joint
    finally:
        for vit, cache, lent in saved:
            vit._feat_cache, vit._grad_arena_lent = cache, lent


def _plan(method, shapes, kw):
    """Argument checks and the (alpha, weight) table of one call: everything that can fail before a launch.  Returns the loop's arguments."""
    score, sign = kw.get("score", "logit"), kw.get("sign", "signed")
    _check_common(score, sign, kw.get("max_batch"), shapes[0][0])
    plan = dict(power=1, level=0.0, seed=None, times_input=bool(kw.get("times_input", False)), sign=sign, score=score,
                max_batch=kw.get("max_batch"), return_pixels=bool(kw.get("return_pixels", False)), endpoints=False)
    if method == "integrated_gradients":
        plan["alphas"], plan["weights"] = path_table(kw.get("steps", 20), kw.get("rule", "trapezoid"))
        noise = kw.get("noise")
        if noise is not None:                        # a noise level, or (noise level, seed): the path points are jittered (SmoothGrad-IG)
            lv, sd = noise if isinstance(noise, (tuple, list)) and len(noise) == 2 else (noise, None)
            plan["level"], plan["seed"] = _check_noise(lv, sd), sd
        plan["times_input"], plan["endpoints"] = True, True
    elif method == "smoothgrad":
        n = _as_int(kw.get("samples", 25), "samples", 1)
        plan["level"], plan["seed"] = _check_noise(kw.get("noise_level", 0.15), kw.get("seed")), kw.get("seed")
        plan["alphas"], plan["weights"], plan["power"] = [1.0] * n, [1.0 / n] * n, 2 if kw.get("squared", False) else 1
    else:
        plan["alphas"], plan["weights"] = [1.0], [1.0]
    return plan


def _run_single(method, model, img, target, baseline, kw):
    shape = _check_img(img, method)
    base = _check_baseline(baseline, shape)
    plan = _plan(method, [shape], kw)
    tgt = check_target(target, shape[0], model._head_width())
    require_cuda(img, base[0] if base[1] else None)
    st = _Stream(model, img, base, True)
    res, _ = _attribute([st], _single_model(model), (model,), shape[0], tgt, **plan)
    return res[0]


def integrated_gradients(model, img, target=None, baseline=None, steps=20, rule="trapezoid", score="logit", sign="signed", noise=None,
                         max_batch=None, return_pixels=False):
    """Integrated gradients of a VisionTransformerMoCo's target score along the straight path from `baseline` to `img`:
    (img - baseline) * sum_s w_s d score / d img at baseline + alpha_s (img - baseline)  ->  AttributionResult.

    steps=20, rule='trapezoid' (steps + 1 points, both ends) | 'midpoint' (steps points); score='logit' | 'prob' (the target's softmax
    probability); sign='signed' | 'abs' (per pixel and channel, before the channels are folded and the patches pooled); baseline: None (zeros,
    the data-set mean after Normalize), a number, one number per channel, or a full (B, 3, H, W) tensor; target: an int, a (B,) integer
    tensor, or None = the argmax of one evaluation forward on img; noise=None, a noise level or (noise level, seed): Gaussian noise on every
    path point as in smoothgrad; max_batch, return_pixels: module docstring."""
    return _run_single("integrated_gradients", model, img, target, baseline,
                       dict(steps=steps, rule=rule, score=score, sign=sign, noise=noise, max_batch=max_batch, return_pixels=return_pixels))


def smoothgrad(model, img, target=None, noise_level=0.15, samples=25, squared=False, seed=None, times_input=False, score="logit", sign="signed",
               max_batch=None, return_pixels=False):
    """SmoothGrad: the mean over `samples`=25 noisy copies img + sigma z of d score / d img (squared=True: of its square), times img with
    times_input=True.  sigma_b = noise_level (max(img_b) - min(img_b)), noise_level=0.15, computed on the device; z: the counter-hash normal
    of mfvit_attr_inputs.  seed=None draws one from torch's CUDA generator; an int seed gives the same bits on every call.  noise_level=0 is
    saliency.  score, sign, target, max_batch, return_pixels as in integrated_gradients."""
    return _run_single("smoothgrad", model, img, target, None,
                       dict(noise_level=noise_level, samples=samples, squared=squared, seed=seed, times_input=times_input, score=score, sign=sign,
                            max_batch=max_batch, return_pixels=return_pixels))


def saliency(model, img, target=None, times_input=False, score="logit", sign="signed", max_batch=None, return_pixels=False):
    """d score / d img of one evaluation forward (times img with times_input=True), folded and pooled as in integrated_gradients."""
    return _run_single("saliency", model, img, target, None,
                       dict(times_input=times_input, score=score, sign=sign, max_batch=max_batch, return_pixels=return_pixels))


def two_stream(method, vits, imgs, out_of, num_classes, mods, target=None, baselines=(None, None), streams="both", **kw):
    """The three methods for a two-stream model (Fus_CrossViT calls this): vits / imgs: the (cxr, enh) encoders and images; out_of(f_cxr,
    f_enh): the model's scored output on the two feature tensors.  Returns ((res_cxr, res_enh), stream_share)."""
    if streams not in STREAMS:
        raise ValueError(f"streams must be one of {STREAMS}, got {streams!r}")
    if not isinstance(baselines, (tuple, list)) or len(baselines) != 2:
        raise ValueError("baselines must be (baseline_cxr, baseline_enh)")
    shapes = [_check_img(img, f"{method} ({n})") for img, n in zip(imgs, ("cxr", "enh"))]
    bases = [_check_baseline(b, s) for b, s in zip(baselines, shapes)]
    plan = _plan(method, shapes, kw)
    tgt = check_target(target, shapes[0][0], num_classes)
    require_cuda(*imgs, *[b[0] if b[1] else None for b in bases])
    sts = [_Stream(v, img, b, streams in ("both", n)) for v, img, b, n in zip(vits, imgs, bases, ("cxr", "enh"))]
    res, joint = _attribute(sts, _two_stream_model(out_of), mods, shapes[0][0], tgt, **plan)
    with torch.no_grad():
        share = (res[0].total if res[0] is not None else torch.zeros_like(joint)) / joint
        share = torch.where(joint == 0, torch.full_like(joint, float("nan")), share)         # no total to share out: NaN
    return (res[0], res[1]), share
