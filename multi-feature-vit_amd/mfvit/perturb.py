"""The perturbation test for patch-relevance maps: which of the project's maps (attention rollout, attention relevance, the exchange's
cross-stream relevance, image gradients pooled per patch) is faithful to the model?

Chefer, Gur & Wolf 2021 section 4 (positive / negative perturbation) and Petsiuk et al. 2018 (deletion / insertion): rank the patches of
every image by relevance, remove them a fraction at a time, run the model again after each removal, and record how the accuracy and the
target class's probability fall.  The area under that curve is the number papers report; for a faithful map positive perturbation falls
fast (low AUC) and negative perturbation slowly (high AUC).  For the two-stream model the same test, run on one stream only, measures what
that stream adds (Fus_CrossViT.perturbation_test with one map None).

Three launches of csrc/perturb.hip do everything but the model forwards, with no host synchronisation:
  patch_rank        (B, P) relevance -> (B, P) int32 rank, most relevant first, a total order that depends on values and indices only:
                    the inverse permutation of np.argsort(-rel, kind="stable") - NaN below -inf, -0.0 ties with +0.0.  NOT
                    torch.argsort(descending=True, stable=True), which puts NaN first.
  perturb_patches   all S masked batches of a test in one launch: out[s] = img with the patches of rank in [lo_s, hi_s) set to fill[c].
  perturb_score     per step: images predicted as the target, sum of the target's softmax probability (double), sum of its logit.
With k patches to remove out of P the three modes are rank ranges: 'positive' [0, k), 'negative' [P - k, P), 'insertion' [k, P) (only
the top k visible).

Limits: patch granularity only (a pixel-level ranking of an upsampled map would need a real sort); the fill is one constant per channel
(no blur or noise fill); one GPU; CPU tensors raise MfvitError like the rest of the package.
"""
import operator

import torch

from ._lib import check, lib, ptr, require_cuda, stream

MAX_PATCHES = 8192          # the project's token limit (include/mfvit.h)
MODES = ("positive", "negative", "insertion")
DEFAULT_FRACTIONS = tuple(i / 10 for i in range(10))


# ---------------------------------------------------------------------------------------------------- host-side tables
def _as_int(v, what):
    try:
        if isinstance(v, bool):
            raise TypeError
        return operator.index(v)
    except TypeError:
        raise ValueError(f"{what} must be an integer, got {v!r}") from None


def step_counts(P, fractions=None, ks=None):
    """The patch counts [k_0, ..] of a test over P patches: k_s = int(P * f_s), truncated as in Chefer's script; fractions default to
    (0, .1, .., .9), must start with 0 and be non-decreasing in [0, 1].  Or ks=: the counts themselves (integers, starting with 0,
    non-decreasing, at most P).  Repeated counts are legal (small P)."""
    P = _as_int(P, "P")
    if not 1 <= P <= MAX_PATCHES:
        raise ValueError(f"P must lie in [1, {MAX_PATCHES}], got {P}")
    if ks is not None:
        if fractions is not None:
            raise ValueError("give fractions or ks, not both")
        out = [_as_int(k, "a patch count") for k in ks]
        if not out or out[0] != 0 or any(b < a for a, b in zip(out, out[1:])) or out[-1] > P:
            raise ValueError(f"ks must start with 0, be non-decreasing and at most P = {P}, got {out}")
        return out
    fr = [float(f) for f in (DEFAULT_FRACTIONS if fractions is None else fractions)]
    if not fr or fr[0] != 0.0 or any(not 0.0 <= f <= 1.0 for f in fr) or any(b < a for a, b in zip(fr, fr[1:])):
        raise ValueError(f"fractions must start with 0 and be non-decreasing in [0, 1], got {fr}")
    return [int(P * f) for f in fr]


def ranges_for(P, ks, mode):
    """The half-open rank ranges [lo_s, hi_s) that remove k_s patches in `mode`, as a CPU int32 [S][2] tensor (the `steps` table of
    mfvit_patch_perturb): 'positive' [0, k) - most relevant first; 'negative' [P - k, P) - least relevant first; 'insertion' [k, P) - only the
    top k stay visible."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    P = _as_int(P, "P")
    ks = [_as_int(k, "a patch count") for k in ks]
    if P < 1 or not ks or any(not 0 <= k <= P for k in ks):
        raise ValueError(f"patch counts must lie in [0, P = {P}], got {ks}")
    if mode == "positive":
        rows = [(0, k) for k in ks]
    elif mode == "negative":
        rows = [(P - k, P) for k in ks]
    else:
        rows = [(k, P) for k in ks]
    return torch.tensor(rows, dtype=torch.int32)


def _check_ranges(ranges, P):
    """ranges as int32 [S][2]; a host-side table (list, CPU tensor) is checked against 0 <= lo <= hi <= P, a device tensor is the caller's
    contract (checking it would synchronise)."""
    r = ranges if isinstance(ranges, torch.Tensor) else torch.as_tensor(ranges)
    if r.dim() != 2 or r.shape[1] != 2 or r.shape[0] < 1 or r.dtype.is_floating_point or r.dtype == torch.bool:
        raise ValueError(f"ranges must be an integer [S][2] table, got {tuple(r.shape)} {r.dtype}")
    if not r.is_cuda and bool(((r[:, 0] < 0) | (r[:, 0] > r[:, 1]) | (r[:, 1] > P)).any()):
        raise ValueError(f"ranges out of order: every row must be 0 <= lo <= hi <= P = {P}, got {r.tolist()}")
    return r.to(torch.int32)


# ---------------------------------------------------------------------------------------------------- thin wrappers
def _map_shape(rel, what):
    if not isinstance(rel, torch.Tensor) or rel.dim() not in (2, 3) or not rel.dtype.is_floating_point:
        raise ValueError(f"{what} must be a floating-point (B, P) or (B, gh, gw) tensor, got "
                         f"{tuple(rel.shape) if isinstance(rel, torch.Tensor) else type(rel).__name__}")
    B, P = int(rel.shape[0]), int(rel[0].numel()) if rel.shape[0] else 0
    if B < 1 or not 1 <= P <= MAX_PATCHES:
        raise ValueError(f"{what}: need B >= 1 and 1 <= P <= {MAX_PATCHES}, got B = {B}, P = {P}")
    return B, P


def _fill_tensor(fill, C, device):
    """fill (None: zeros; one number; C numbers) as a contiguous f32 [C] tensor on `device`.  A tensor already there is used as it is: no copy."""
    if fill is None:
        return torch.zeros(C, dtype=torch.float32, device=device)
    f = (fill.detach() if isinstance(fill, torch.Tensor) else torch.as_tensor(fill)).to(torch.float32).reshape(-1)
    if f.numel() == 1:
        f = f.expand(C)
    if f.numel() != C:
        raise ValueError(f"fill must be None, one number or {C} numbers (one per channel), got {f.numel()}")
    return f.to(device).contiguous()


def patch_rank(rel):
    """rel (B, P) or (B, gh, gw), any float dtype (cast to f32) -> int32 (B, P): rank[b][i] = the position of patch i of image b, most
    relevant first; rank[i] = #{j : rel[j] > rel[i], or rel[j] == rel[i] and j < i}, NaN below every number (module docstring)."""
    B, P = _map_shape(rel, "rel")
    require_cuda(rel)
    r = rel.detach().reshape(B, P).float()
    if r.stride(1) != 1 or r.stride(0) < P:
        r = r.contiguous()
    rank = torch.empty(B, P, device=r.device, dtype=torch.int32)
    check(lib().mfvit_patch_rank(ptr(r), r.stride(0), ptr(rank), B, P, stream()), "mfvit_patch_rank")
    return rank


def perturb_patches(img, rank, ranges, fill=None):
    """img (B, C, H, W) with H, W multiples of 16, rank int32 (B, P) as patch_rank returns it, ranges an integer [S][2] table (ranges_for) ->
    f32 (S, B, C, H, W): out[s] = img with the patches whose rank lies in [lo_s, hi_s) set to fill[c].  fill: None (zeros, the data-set
    mean after Normalize), a number, or C numbers.  Moves and fills only: bit-exact."""
    if not isinstance(img, torch.Tensor) or img.dim() != 4:
        raise ValueError(f"img must be a (B, C, H, W) tensor, got {tuple(img.shape) if isinstance(img, torch.Tensor) else type(img).__name__}")
    B, C, H, W = (int(v) for v in img.shape)
    if B < 1 or C < 1 or H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError(f"img must hold at least one image with H and W positive multiples of 16, got {tuple(img.shape)}")
    P = (H // 16) * (W // 16)
    if P > MAX_PATCHES:
        raise ValueError(f"{P} patches exceed the limit of {MAX_PATCHES}")
    if not isinstance(rank, torch.Tensor) or tuple(rank.shape) != (B, P) or rank.dtype != torch.int32:
        raise ValueError(f"rank must be an int32 ({B}, {P}) tensor, got "
                         f"{(tuple(rank.shape), rank.dtype) if isinstance(rank, torch.Tensor) else type(rank).__name__}")
    steps = _check_ranges(ranges, P)
    f = _fill_tensor(fill, C, img.device)
    require_cuda(img, rank)
    x = img.detach().float().contiguous()
    rank, steps = rank.contiguous(), steps.to(x.device).contiguous()
    S = int(steps.shape[0])
    out = torch.empty(S, B, C, H, W, device=x.device, dtype=torch.float32)
    check(lib().mfvit_patch_perturb(ptr(x), ptr(rank), ptr(steps), ptr(f), ptr(out), B, C, H, W, S, stream()), "mfvit_patch_perturb")
    return out


def perturb_score(logits, target, correct, sums, nonfinite):
    """logits f32 (S, B, C), target int64 (B,) with classes in [0, C) (the caller's contract).  ACCUMULATES per step into correct int64 [S]
    (images whose first-maximum argmax is the target), sums f64 [S][2] (the target's softmax probability, computed in double, and its
    raw logit) and nonfinite int64 [S] (rows with a non-finite logit: wrong, 0 to both sums).  One launch, a fixed-order sum."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError("perturb_score: logits must be an f32 (S, B, C) tensor")
    S, B, C = (int(v) for v in logits.shape)
    if S < 1 or B < 1 or C < 1:
        raise ValueError(f"perturb_score: empty logits {tuple(logits.shape)}")
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (B,) or target.dtype != torch.int64:
        raise ValueError(f"perturb_score: target must be an int64 ({B},) tensor")
    if tuple(correct.shape) != (S,) or correct.dtype != torch.int64 or tuple(nonfinite.shape) != (S,) or nonfinite.dtype != torch.int64 \
            or tuple(sums.shape) != (S, 2) or sums.dtype != torch.float64:
        raise ValueError(f"perturb_score: the accumulators must be int64 [{S}], f64 [{S}][2] and int64 [{S}]")
    require_cuda(logits, target, correct, sums, nonfinite)
    if not (correct.is_contiguous() and sums.is_contiguous() and nonfinite.is_contiguous()):
        raise ValueError("perturb_score: the accumulators must be contiguous (they are updated in place)")
    z = logits.detach()
    if z.stride(2) != 1 or z.stride(1) < C or z.stride(0) != B * z.stride(1):
        z = z.contiguous()
    check(lib().mfvit_perturb_score(ptr(z), z.stride(1), ptr(target.contiguous()), S, B, C, ptr(correct), ptr(sums), ptr(nonfinite), stream()),
          "mfvit_perturb_score")


# ---------------------------------------------------------------------------------------------------- the meter
def _trapezoid(y, x):
    """The trapezoid area of y over x divided by the span of x (float64, plain Python); nan for an empty span."""
    span = x[-1] - x[0]
    if not span > 0:
        return float("nan")
    return sum((x[i + 1] - x[i]) * (y[i + 1] + y[i]) * 0.5 for i in range(len(x) - 1)) / span


class PerturbationResult:
    """Per-step lists accuracy, mean_prob, mean_logit, nonfinite and fractions (k_s / P actually used; None when the meter was never told),
    the image count n, and auc_accuracy / auc_prob: the trapezoid over the fractions divided by their span (None without fractions)."""

    def __init__(self, accuracy, mean_prob, mean_logit, fractions, n, nonfinite):
        self.accuracy, self.mean_prob, self.mean_logit, self.fractions, self.n, self.nonfinite = accuracy, mean_prob, mean_logit, fractions, n, nonfinite
        self.auc_accuracy = _trapezoid(accuracy, fractions) if fractions is not None else None
        self.auc_prob = _trapezoid(mean_prob, fractions) if fractions is not None else None

    def as_dict(self):
        return dict(self.__dict__)

    def __repr__(self):
        return f"PerturbationResult({self.as_dict()})"


class PerturbationMeter:
    """Accumulates the scores of a perturbation test over the batches of a data set, on the device:

        meter = PerturbationMeter(num_steps=10)
        for img, label in loader:  perturbation_test(model, img, model.attention_relevance(img), target=label, meter=meter)
        res = meter.compute()            # ONE device-to-host copy; res.auc_prob, res.accuracy, ..

    update() launches mfvit_perturb_score and never synchronises; every batch must use the same steps."""

    def __init__(self, num_steps, fractions=None):
        self.num_steps = _as_int(num_steps, "num_steps")
        if self.num_steps < 1:
            raise ValueError(f"num_steps must be positive, got {num_steps}")
        self.fractions = None
        if fractions is not None:
            self.set_fractions(fractions)
        self.reset()

    def set_fractions(self, fractions):
        """The fractions k_s / P of the steps, for the AUC; a meter keeps the ones it was given first and refuses different ones."""
        fr = [float(f) for f in fractions]
        if len(fr) != self.num_steps:
            raise ValueError(f"{len(fr)} fractions for a meter of {self.num_steps} steps")
        if self.fractions is not None and fr != self.fractions:
            raise ValueError(f"this meter accumulates a curve over the fractions {self.fractions}, got {fr}")
        self.fractions = fr

    def reset(self):
        self._buf = None            # int64 [4 S]: correct | nonfinite | the f64 sums [S][2] (one buffer: one copy in compute())
        self.n = 0

    def _views(self):
        S = self.num_steps
        return self._buf[:S], self._buf[S:2 * S], self._buf[2 * S:].view(torch.float64).view(S, 2)

    def update(self, logits, target):
        """logits f32 (S, B, C) on the device; target int64 (B,) (a CPU tensor is checked against [0, C) and copied; a device tensor is the
        caller's contract).  No host synchronisation."""
        if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.shape[0] != self.num_steps:
            raise ValueError(f"update: logits must be (S = {self.num_steps}, B, C), got "
                             f"{tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
        if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or tuple(target.shape) != (int(logits.shape[1]),):
            raise ValueError(f"update: target must be an int64 ({int(logits.shape[1])},) tensor")
        if not target.is_cuda and target.numel() and (int(target.min()) < 0 or int(target.max()) >= logits.shape[2]):
            raise ValueError(f"update: target class out of range for {int(logits.shape[2])} classes: {target.tolist()}")
        require_cuda(logits)
        if self._buf is None:
            self._buf = torch.zeros(4 * self.num_steps, device=logits.device, dtype=torch.int64)
        correct, nonfinite, sums = self._views()
        perturb_score(logits.float(), target.to(logits.device), correct, sums, nonfinite)
        self.n += int(logits.shape[1])

    @staticmethod
    def result_from(correct, nonfinite, sums, n, fractions=None):
        """The result object from accumulator contents on the host (lists / CPU tensors): float64 throughout."""
        correct, nonfinite = [int(v) for v in correct], [int(v) for v in nonfinite]
        sums = [[float(a), float(b)] for a, b in sums]
        n = int(n)
        if n < 1:
            raise ValueError("no image was scored")
        return PerturbationResult([c / n for c in correct], [s[0] / n for s in sums], [s[1] / n for s in sums],
                                  None if fractions is None else [float(f) for f in fractions], n, nonfinite)

    def compute(self):
        if self._buf is None:
            raise ValueError("compute() before the first update()")
        S = self.num_steps
        host = self._buf.cpu()                                                      # the one copy
        return self.result_from(host[:S].tolist(), host[S:2 * S].tolist(), host[2 * S:].view(torch.float64).view(S, 2).tolist(), self.n,
                                self.fractions)


# ---------------------------------------------------------------------------------------------------- the test itself
def _plan(img, maps, fractions, ks, mode, max_batch, what):
    """Argument checks and host tables of one stream: (B, P, counts) for an image batch and its map (None: the stream stays intact)."""
    if not isinstance(img, torch.Tensor) or img.dim() != 4:
        raise ValueError(f"{what}: the images must be a (B, C, H, W) tensor")
    B, _, H, W = (int(v) for v in img.shape)
    if B < 1 or H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError(f"{what}: need at least one image with H and W positive multiples of 16, got {tuple(img.shape)}")
    P = (H // 16) * (W // 16)
    if maps is not None:
        mb, mp = _map_shape(maps, f"{what}: the map")
        if (mb, mp) != (B, P) or (maps.dim() == 3 and tuple(maps.shape[1:]) != (H // 16, W // 16)):
            raise ValueError(f"{what}: the map must be ({B}, {H // 16}, {W // 16}) or ({B}, {P}), got {tuple(maps.shape)}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if max_batch is not None and _as_int(max_batch, "max_batch") < B:
        raise ValueError(f"max_batch = {max_batch} is smaller than the batch ({B} images): steps are forwarded whole")
    return B, P, step_counts(P, fractions, ks)


def _groups(S, B, max_batch):
    """[(s0, s1)): the steps of every forward - whole steps, at most max_batch images."""
    g = max(1, (B if max_batch is None else int(max_batch)) // B)
    return [(s, min(s + g, S)) for s in range(0, S, g)]


def _meter_for(meter, ks, P):
    S = len(ks)
    if meter is None:
        meter = PerturbationMeter(S)
    elif not isinstance(meter, PerturbationMeter) or meter.num_steps != S:
        raise ValueError(f"meter must be a PerturbationMeter of {S} steps")
    meter.set_fractions([k / P for k in ks])
    return meter


def run_steps(forward, streams, S, B, max_batch, tgt, meter, need_clean):
    """The shared loop of the single- and two-stream tests.  streams: [(img, rank or None, ranges, fill)]; forward(list of (g * B, C, H, W)
    batches) -> (g * B, classes) logits.  tgt: CPU int64 (B,) or None (the model's prediction on the unperturbed images: step 0, or one
    more forward when need_clean says step 0 is perturbed).  Returns the (S, B, classes) logits."""
    logits = None
    # (the tables were built by ranges_for: they go to the device once, and a device table is not checked again)
    # and so does the fill: the loop below copies nothing from the host
    streams = [(img, rank, None if rank is None else ranges.to(img.device), None if rank is None else _fill_tensor(fill, int(img.shape[1]), img.device))
               for img, rank, ranges, fill in streams]
    for s0, s1 in _groups(S, B, max_batch):
        xs = []
        for img, rank, ranges, fill in streams:
            if rank is None:
                x = img.detach().float().contiguous()
                xs.append(x if s1 - s0 == 1 else x.repeat(s1 - s0, 1, 1, 1))
            else:
                xs.append(perturb_patches(img, rank, ranges[s0:s1], fill).flatten(0, 1))
        out = forward(xs).detach().float()
        if logits is None:
            logits = torch.empty(S, B, out.shape[1], device=out.device, dtype=torch.float32)
        logits[s0:s1] = out.view(s1 - s0, B, -1)
    if tgt is None:
        clean = forward([img.detach().float().contiguous() for img, _, _, _ in streams]).detach() if need_clean else logits[0]
        tgt_dev = clean.argmax(dim=1)
    else:
        if tgt.numel() and int(tgt.max()) >= logits.shape[2]:
            raise ValueError(f"target class out of range for {logits.shape[2]} classes: {tgt.tolist()}")
        tgt_dev = tgt.to(logits.device)
    meter.update(logits, tgt_dev)
    return logits


def perturbation_test(model, img, maps, target=None, fractions=None, mode="positive", fill=None, max_batch=None, meter=None,
                      return_logits=False, ks=None):
    """The perturbation test of one relevance map on a VisionTransformerMoCo: meter, or (meter, logits (S, B, classes)) with return_logits.

    maps: (B, gh, gw) or (B, P) relevance from any source (attention_rollout, attention_relevance, pooled image gradients ..).  The patches
    are ranked (patch_rank), step s masks k_s = int(P * fractions[s]) of them (step_counts; ks= gives the counts instead) in `mode`
    ('positive': most relevant first, 'negative': least relevant first, 'insertion': only the top k_s visible) with `fill` (perturb_patches),
    and the model's ordinary evaluation forward scores every masked batch.  Step 0 removes nothing, so in the two removal modes it is the
    unperturbed forward.  target: an int or a (B,) integer tensor, or None: the model's prediction on the unperturbed images (Chefer's
    "predicted" variant) - the argmax of step 0, or of one more forward in 'insertion' mode, whose step 0 hides everything.

    max_batch bounds the images per forward (default B: one step per forward, S forwards); steps are forwarded whole, so max_batch >= B.
    The encoder picks kernels by row count: the logits are bit-reproducible for a fixed max_batch, not across different ones.

    Runs under no_grad with the model in evaluation mode; training flags, RNG state, the feature cache and p.grad stay as they were.  The
    meter is updated (created when None) without a host synchronisation unless the target is given (its class range is checked)."""
    from .encoder import check_target, eval_modules
    B, P, counts = _plan(img, maps, fractions, ks, mode, max_batch, "perturbation_test")
    if maps is None:
        raise ValueError("perturbation_test: maps is required")
    tgt = check_target(target, B, model._head_width())
    meter = _meter_for(meter, counts, P)
    require_cuda(img, maps)
    saved = (model._feat_cache, getattr(model, "_grad_arena_lent", False))
    try:
        with torch.no_grad(), eval_modules(model):
            rank = patch_rank(maps)
            logits = run_steps(lambda xs: model(xs[0]), [(img, rank, ranges_for(P, counts, mode), fill)], len(counts), B, max_batch, tgt, meter,
                               mode == "insertion")
    finally:
        model._feat_cache, model._grad_arena_lent = saved
    return (meter, logits) if return_logits else meter
