"""Gradient attribution on the GPU (include/mfvit.h: mfvit_attr_inputs, mfvit_attr_accumulate, mfvit_attr_finish; csrc/attribution.hip;
mfvit.attribution) against the numpy / float64 restatements of tests/attribution_ref.py.

The three kernels are held to the gates derived in attribution_ref's docstring from their operation orders; every output sits between NaN
guard bands and every kernel test runs once 16 bytes and once 4 bytes behind its allocations (the 16-byte and the scalar path).

The end-to-end gate (encoder and two-stream model against oracle.ref_vit / oracle.ref_fusion in float64 on the same path points and the same
noise) cannot be derived: it is the TOL of tests/test_input_grad_gpu.py for the precision, the image gradient's own gate, and at least
2 x the error measured on one MI355X (largest over maps, pixels, total and scores, all cases of a precision; profiles/attribution_bench.txt):
    bf16x3 3.1e-4 at 224^2 and 2.7e-4 at 64^2 (gate 1e-3), fp32 2.0e-6 (gate 1e-5), fp16 1.8e-3 (gate 1e-2);
    Fus_CrossViT in bf16x3: 2.6e-4 ('both'), 2.4e-4 ('cxr'), 1.5e-4 ('enh') (gate 1e-3)."""
import importlib
import math

import numpy as np
import pytest
import torch

import attribution_ref as R
from conftest import rng_tensor
from mfvit import attribution as A          # (at module level: without the feature every test here fails)
from oracle import ref_fusion, ref_vit

DEV = "cuda:0"
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
TOL = {"fp32": 1e-5, "bf16x3": 1e-3, "fp16": 1e-2}          # tests/test_input_grad_gpu.py
PROF_GEMM_TN = 3                                             # kernel class of the weight-gradient GEMMs (mfvit_prof_*)
GUARD = 256
SHAPES = [(2, 3, 16, 16), (3, 3, 32, 48), (2, 1, 48, 32)]
ALPHA = np.array([0.0, 1.0, 0.5, 1.0 / 3.0], dtype=np.float32)


def _a():
    return A


def _L():
    from mfvit import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _put(arr, off):
    """arr on the device `off` bytes behind a NaN-filled allocation: (keep-alive tensor, device pointer)."""
    o = off // 4
    t = torch.full((o + arr.size,), float("nan"), dtype=torch.float32, device=DEV)
    t[o:] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).reshape(-1).to(DEV)
    return t, t.data_ptr() + 4 * o


def _banded(n, off, dtype=torch.float32, fill=float("nan")):
    """An output of n elements `off` bytes behind an allocation, between guard bands: (tensor, pointer, read() -> (values, guards intact))."""
    o = off // 4 if dtype == torch.float32 else 0
    t = torch.full((o + GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)

    def read():
        h = t.cpu().numpy()
        return h[o + GUARD:o + GUARD + n].copy(), bool(np.isnan(h[:o + GUARD]).all() and np.isnan(h[o + GUARD + n:]).all())
    return t, t.data_ptr() + t.element_size() * (o + GUARD), read


def _case(shape, seed, full):
    g = _rng(seed)
    x = g.standard_normal(shape).astype(np.float32)
    base = (g.standard_normal(shape) if full else (0.5 + np.arange(shape[1])) * -1.25).astype(np.float32)
    return x, base


def _violations(got, ref, gate):
    d = np.abs(got.astype(np.float64) - ref)
    print(f"    max |got - ref| {d.max():.3e}, largest share of the gate {np.max(d / np.maximum(gate, 1e-300)):.3f}")
    return int((d > gate).sum())


# ------------------------------------------------------------------------------------------------ 1. inputs
def _run_inputs(x, base, alpha, off, sigma=None, seed=None, s0=0):
    L = _L()
    S, (B, C, H, W) = len(alpha), x.shape
    kx, px = _put(x, off)
    kb, pb = _put(base, off if base.ndim == 4 else 0)
    ka, pa = _put(alpha, 0)
    ks, ps = _put(sigma, 0) if sigma is not None else (None, None)
    sd = torch.tensor([seed], dtype=torch.int64, device=DEV) if seed is not None else None
    out, po, read = _banded(S * x.size, off)
    L.check(L.lib().mfvit_attr_inputs(px, pb, int(base.ndim == 4), pa, ps, None if sd is None else sd.data_ptr(), s0, po, S, B, C, H * W, _stream()),
            "mfvit_attr_inputs")
    got, intact = read()
    return got.reshape((S,) + x.shape), intact


@pytest.mark.gpu
@pytest.mark.parametrize("off", [16, 4])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_inputs_are_within_the_gate_and_the_end_points_bit_exact(shape, full, off):
    x, base = _case(shape, sum(shape), full)
    ref = R.ref_inputs(x, base, ALPHA)
    got, intact = _run_inputs(x, base, ALPHA, off)
    assert intact, "a guard band was written"
    assert np.array_equal(got[0], R._base_like(base, x).astype(np.float32)) and np.array_equal(got[1], x)      # alpha 0 and 1: moves
    assert _violations(got, ref, R.gate_inputs(x, base, ALPHA, ref)) == 0
    again, _ = _run_inputs(x, base, ALPHA, off)
    assert again.tobytes() == got.tobytes()
    if off == 16:                                                                 # the wrapper, on aligned tensors
        a = _a()
        out = a.attr_inputs(torch.from_numpy(x).to(DEV), torch.from_numpy(base).to(DEV), torch.from_numpy(ALPHA).to(DEV))
        assert out.shape == (4,) + shape and out.cpu().numpy().tobytes() == got.tobytes()


@pytest.fixture(scope="module")
def noise():
    """The noise itself, exported at (4, 3, 224, 224), four samples: x = 0, base = 0, alpha = 1, sigma = 1."""
    shape, seed = (4, 3, 224, 224), 20241019
    zero, one = np.zeros(shape, np.float32), np.ones(4, np.float32)
    got, intact = _run_inputs(zero, np.zeros(3, np.float32), one, 16, sigma=one, seed=seed)
    return shape, seed, zero, one, got, intact, R.ref_noise(seed, 0, 4, shape)


@pytest.mark.gpu
def test_exported_noise_matches_the_float64_restatement(noise):
    """Gate (attribution_ref.gate_normal): 9 * 2^-24 |z| from the documented ulp bounds of logf, sqrtf and cospif."""
    shape, seed, zero, one, got, intact, ref = noise
    assert intact and np.isfinite(got).all()
    assert _violations(got, ref, R.gate_normal(ref)) == 0
    n = got.size
    z = got.astype(np.float64)
    mean, var = z.mean(), z.var()
    print(f"[noise] n {n}: mean {mean:.3e} (bound {5 / math.sqrt(n):.3e}), var - 1 {var - 1:.3e} (bound {5 * math.sqrt(2 / n):.3e})")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)


@pytest.mark.gpu
def test_noise_does_not_depend_on_the_grouping_and_scales_with_sigma(noise):
    shape, seed, zero, one, got, _, _ = noise
    first, _ = _run_inputs(zero, np.zeros(3, np.float32), one[:2], 16, sigma=one, seed=seed)
    second, _ = _run_inputs(zero, np.zeros(3, np.float32), one[:2], 16, sigma=one, seed=seed, s0=2)
    assert first.tobytes() == got[:2].tobytes() and second.tobytes() == got[2:].tobytes()
    scalar, _ = _run_inputs(zero, np.zeros(3, np.float32), one[:1], 4, sigma=one, seed=seed, s0=3)     # the scalar path: the same noise
    assert scalar.tobytes() == got[3:].tobytes()
    # out = fmaf(sigma_b, z, v) on a path point: one more rounding than the noise-free point
    x, base = _case(shape, 5, False)
    sigma = np.array([0.0, 0.5, 1.0, 2.5], np.float32)
    al = np.array([1.0, 0.25], np.float32)
    out, _ = _run_inputs(x, base, al, 16, sigma=sigma, seed=seed, s0=1)
    zz = got[1:3].astype(np.float64)                                               # the kernel's own z of samples 1 and 2
    ref = R.ref_inputs(x, base, al, sigma, zz)
    gate = R.U * R.SLACK * (np.abs(al.astype(np.float64)).reshape(-1, 1, 1, 1, 1) * np.abs(x.astype(np.float64) - R._base_like(base, x)) + np.abs(ref)
                            + np.abs(ref - sigma.reshape(1, -1, 1, 1, 1) * zz))
    assert _violations(out, ref, gate) == 0
    assert np.array_equal(out[0, 0], x[0])                                        # sigma = 0, alpha = 1: the image itself


# ------------------------------------------------------------------------------------------------ 2. accumulate and finish
def _run_accumulate(grad, w, off, acc0=None):
    L = _L()
    k, B = grad.shape[:2]
    n = grad[0, 0].size
    kg, pg = _put(grad, off)
    kw, pw = _put(w, 0)
    out, po, read = _banded(B * n, off)
    out[(off // 4) + GUARD:(off // 4) + GUARD + B * n] = 0.0 if acc0 is None else torch.from_numpy(acc0).reshape(-1).to(DEV)
    return L, pg, pw, po, k, B, n, read, (kg, kw, out)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [16, 4])
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("shape", SHAPES + [(2, 3, 224, 224)])
def test_accumulate_is_within_k_roundings_of_the_float64_sum(shape, k, power, off):
    """Gate (attribution_ref.gate_accumulate): k * 2^-24 * sum_s |w_s g^p|."""
    g = _rng(sum(shape) + k)
    grad = g.standard_normal((k,) + shape).astype(np.float32)
    w = (g.random(k) + 0.1).astype(np.float32)
    runs = []
    for _ in range(2):
        L, pg, pw, po, kk, B, n, read, keep = _run_accumulate(grad, w, off)
        L.check(L.lib().mfvit_attr_accumulate(pg, pw, po, kk, B, n, power, _stream()), "mfvit_attr_accumulate")
        got, intact = read()
        assert intact, "a guard band was written"
        runs.append(got)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert _violations(runs[0].reshape(shape), R.ref_accumulate(grad, w, power), R.gate_accumulate(grad, w, power)) == 0
    if off == 16 and k == 3:
        # two groups (steps 0, 1 then step 2) against one of three: the chain is the same, so are the bits
        a = _a()
        gd, wd = torch.from_numpy(grad).to(DEV), torch.from_numpy(w).to(DEV)
        one, two = torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV)
        a.attr_accumulate(gd, wd, one, power)
        a.attr_accumulate(gd[:2], wd[:2], two, power)
        a.attr_accumulate(gd[2:], wd[2:], two, power)
        assert torch.equal(one, two) and one.cpu().numpy().tobytes() == runs[0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("off", [16, 4])
@pytest.mark.parametrize("absval", [False, True])
@pytest.mark.parametrize("times_input", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(2, 3, 224, 224)])
def test_finish_is_within_its_summation_tree_of_the_float64_sums(shape, times_input, absval, off):
    """Gates (attribution_ref.gate_finish): pixels (2 + C - 1) 2^-24 sum_c |t_c|, patches 8 more roundings over the patch's terms (the 2 only
    with times_input); total within 1e-12 of the exact sum of the kernel's f32 terms, relative to sum |t|."""
    L = _L()
    B, C, H, W = shape
    g = _rng(sum(shape) + 7)
    acc = g.standard_normal(shape).astype(np.float32)
    full = sum(shape) % 2 == 0
    x, base = _case(shape, sum(shape) + 8, full)
    args = (acc, x, base) if times_input else (acc,)
    px, pt, tot, mag_px, mag_pt = R.ref_finish(*args, absval=absval)
    g_px, g_pt = R.gate_finish(C, times_input, mag_px, mag_pt)
    exact, mag = R.exact_total(R.f32_terms(*args))
    runs = []
    for _ in range(2):
        ka, pa = _put(acc, off)
        kx, pxx = _put(x, off)
        kb, pb = _put(base, off if full else 0)
        o_px, p_px, r_px = _banded(B * H * W, off)
        o_pt, p_pt, r_pt = _banded(B * (H // 16) * (W // 16), off)
        o_tt, p_tt, r_tt = _banded(B, 0, torch.float64)
        L.check(L.lib().mfvit_attr_finish(pa, pxx if times_input else None, pb if times_input else None, int(full), int(times_input), int(absval),
                                          p_px, p_pt, p_tt, B, C, H, W, _stream()), "mfvit_attr_finish")
        runs.append([r() for r in (r_px, r_pt, r_tt)])
        assert all(r[1] for r in runs[-1]), "a guard band was written"
    for a, b in zip(runs[0], runs[1]):
        assert a[0].tobytes() == b[0].tobytes()
    got_px, got_pt, got_tot = (r[0] for r in runs[0])
    assert _violations(got_px.reshape(B, H, W), px, g_px) == 0
    assert _violations(got_pt.reshape(pt.shape), pt, g_pt) == 0
    for b in range(B):
        print(f"    total[{b}] {got_tot[b]!r} exact {exact[b]!r} rel {abs(got_tot[b] - exact[b]) / mag[b]:.2e}")
    assert (np.abs(got_tot - exact) <= R.SUM_TOL * mag).all()
    assert (np.abs(got_tot - tot) <= 2 * R.U * R.SLACK * mag).all()
    if off == 16:                                                                 # the wrapper, with and without the pixel map
        a = _a()
        ad, xd, bd = (torch.from_numpy(v).to(DEV) for v in (acc, x, base))
        m1, p1, t1 = a.attr_finish(ad, xd if times_input else None, bd if times_input else None, absval, True)
        m2, p2, t2 = a.attr_finish(ad, xd if times_input else None, bd if times_input else None, absval, False)
        assert p2 is None and torch.equal(m1, m2) and torch.equal(t1, t2) and t1.dtype == torch.float64
        assert m1.cpu().numpy().tobytes() == got_pt.tobytes() and p1.cpu().numpy().tobytes() == got_px.tobytes()


# ------------------------------------------------------------------------------------------------ 3. one encoder, end to end
def build(depth=2, precision="bf16x3", seed=7, img_size=224, **kw):
    import vits
    m = vits.vit_small(num_classes=3, depth=depth, precision=precision, img_size=img_size, **kw)
    sd = ref_vit.seeded_params(seed, num_classes=3, depth=depth)
    sd["pos_embed"] = m.pos_embed.detach().clone()
    m.load_state_dict(sd)
    return m.to(DEV), sd


def _oracle(logits_fn, tgt, score="logit"):
    """score_and_grad over float64 points for attribution_ref: logits_fn(list of float64 tensors) -> (N, classes)."""
    def f(*points):
        xs = [torch.from_numpy(np.ascontiguousarray(p)).requires_grad_(True) for p in points]
        out = logits_fn(*xs)
        sc = (out.softmax(dim=1) if score == "prob" else out).gather(1, tgt.view(-1, 1)).view(-1)
        gs = torch.autograd.grad(sc.sum(), xs)
        return sc.detach().numpy(), [g.numpy() for g in gs]
    return f


def _sigma(x, level):
    """sigma_b as mfvit.attribution forms it on the device."""
    xd = x.to(DEV)
    return ((xd.amax(dim=(1, 2, 3)) - xd.amin(dim=(1, 2, 3))) * level).contiguous()


def _exported_noise(shape, samples, seed):
    a = _a()
    B, C = shape[:2]
    z = a.attr_inputs(torch.zeros(shape, device=DEV), torch.zeros(C, device=DEV), torch.ones(samples, device=DEV), torch.ones(B, device=DEV),
                      torch.tensor([seed], dtype=torch.int64, device=DEV))
    return z.double().cpu().numpy()


def _pool(attr):
    px = attr.sum(axis=1)
    return px, R._patch_sum(px), attr.sum(axis=(1, 2, 3)), np.abs(attr).sum(axis=(1, 2, 3))


def _f32_table(values):
    return np.asarray(values, dtype=np.float32).astype(np.float64)


SG_SEED, SG_LEVEL, SG_SAMPLES, STEPS = 4711, 0.15, 4, 8
_REFS = {}


def single_refs(size):
    """The float64 restatements of the three end-to-end cases at one image size, computed once: the same weights, images, path points (the f32
    tables the kernel reads) and noise (exported by the kernel) through oracle.ref_vit.forward."""
    if size in _REFS:
        return _REFS[size]
    m, sd = build(img_size=size)
    B = 3
    img = rng_tensor(61 + size, (B, 3, size, size))
    tgt = torch.tensor([2, 0, 1])
    pd = {k: v.double() for k, v in sd.items()}
    f1 = _oracle(lambda x: ref_vit.forward(pd, x), tgt)
    f = lambda p: (lambda s, g: (s, g[0]))(*f1(p))                               # noqa: E731
    x64 = img.double().numpy()
    base = np.array([0.1, -0.2, 0.3], np.float32)
    b64 = R._base_like(base, x64).astype(np.float64)
    out = {"img": img, "tgt": tgt, "base": base}
    for rule in ("trapezoid", "midpoint"):
        al, w = R.path_points(STEPS, rule)
        attr, s1, s0 = R.integrated_gradients(f, x64, b64, _f32_table(al), _f32_table(w))
        out[rule] = (_pool(attr), s1, s0)
    z = _exported_noise(img.shape, SG_SAMPLES, SG_SEED)
    sg = _sigma(img, SG_LEVEL).double().cpu().numpy().reshape(1, B, 1, 1, 1)
    out["smoothgrad"] = (_pool(R.smoothgrad(f, x64, sg * z)), None, None)
    _REFS[size] = out
    return out


def _errors(res, ref, own_delta=True):
    """max |got - ref| / max |ref| of maps, pixels and scores; the total's error over the oracle's sum |attribution|."""
    (px, pt, tot, mag), s1, s0 = ref
    r = res.cpu()

    def rel(got, want):
        return float(np.abs(got.double().numpy() - want).max() / np.abs(want).max())
    e = {"maps": rel(r.maps, pt), "pixels": rel(r.pixels, px), "total": float((np.abs(r.total.numpy() - tot) / mag).max())}
    if s1 is not None:
        e["score_input"], e["score_baseline"] = rel(r.score_input, s1), rel(r.score_baseline, s0)
        assert not own_delta or torch.equal(r.delta, r.total - (r.score_input - r.score_baseline))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("size,precision", [(64, "bf16x3"), (224, "bf16x3"), (224, "fp32"), (224, "fp16")])
def test_encoder_attributions_match_the_float64_restatement(size, precision):
    a = _a()
    ref = single_refs(size)
    m, _ = build(img_size=size, precision=precision)
    x, tgt, base = ref["img"].to(DEV), ref["tgt"], ref["base"]
    calls = {"trapezoid": lambda: a.integrated_gradients(m, x, tgt, base.tolist(), steps=STEPS, rule="trapezoid", return_pixels=True),
             "midpoint": lambda: a.integrated_gradients(m, x, tgt, torch.from_numpy(base), steps=STEPS, rule="midpoint", return_pixels=True),
             "smoothgrad": lambda: a.smoothgrad(m, x, tgt, noise_level=SG_LEVEL, samples=SG_SAMPLES, seed=SG_SEED, return_pixels=True)}
    worst = 0.0
    for name, call in calls.items():
        res = call()
        assert res.maps.shape == (3, size // 16, size // 16) and res.maps.dtype == torch.float32 and res.pixels.shape == (3, size, size)
        assert res.total.dtype == torch.float64 and res.total.shape == (3,) and res.maps.is_cuda
        e = _errors(res, ref[name])
        print(f"[{precision} {size} {name}] " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
        worst = max(worst, max(e.values()))
        again = call()
        assert torch.equal(again.maps, res.maps) and torch.equal(again.pixels, res.pixels) and torch.equal(again.total, res.total)
        if name == "trapezoid":
            d = res.cpu()
            print(f"    completeness: delta {d.delta.tolist()} of {(d.score_input - d.score_baseline).tolist()}")
    print(f"[{precision} {size}] worst {worst:.2e} (gate {TOL[precision]:.0e})")
    assert worst < TOL[precision], worst


@pytest.mark.gpu
def test_grouping_forms_and_scores_of_the_encoder_calls():
    a = _a()
    ref = single_refs(64)
    m, _ = build(img_size=64)
    x, tgt = ref["img"].to(DEV), ref["tgt"]
    B = 3
    one = a.integrated_gradients(m, x, tgt, steps=4, return_pixels=True)
    # max_batch = 2 B (+ 1): two steps per forward - the same method at another batch size, not the same bits
    two = a.integrated_gradients(m, x, tgt, steps=4, max_batch=2 * B + 1, return_pixels=True)
    assert float((one.pixels - two.pixels).abs().max() / one.pixels.abs().max()) < TOL["bf16x3"]
    again = a.integrated_gradients(m, x, tgt, steps=4, max_batch=2 * B + 1, return_pixels=True)
    assert torch.equal(again.pixels, two.pixels) and torch.equal(again.total, two.total)
    # sign='abs': maps of the absolute terms, the total stays signed
    ab = a.integrated_gradients(m, x, tgt, steps=4, sign="abs", return_pixels=True)
    assert torch.equal(ab.total, one.total) and bool((ab.pixels >= one.pixels.abs()).all()) and bool((ab.maps >= 0).all())
    # target None: the argmax of one evaluation forward; a device target; score='prob'
    with torch.no_grad():
        was = m.training
        m.eval()
        pred = m(x).argmax(dim=1)
        m.train(was)
    auto, given = a.saliency(m, x), a.saliency(m, x, pred)
    assert torch.equal(auto.maps, given.maps) and auto.pixels is None and auto.score_input is None and auto.delta is None
    pr = a.integrated_gradients(m, x, tgt, steps=4, score="prob").cpu()
    assert bool(((pr.score_input > 0) & (pr.score_input < 1) & (pr.score_baseline > 0) & (pr.score_baseline < 1)).all())
    # a full-tensor baseline equal to the per-channel one: the same bits; the midpoint rule takes its end points from two more forwards
    full = torch.tensor([0.1, -0.2, 0.3], device=DEV).view(1, 3, 1, 1).expand_as(x).contiguous()
    c1 = a.integrated_gradients(m, x, tgt, [0.1, -0.2, 0.3], steps=3, rule="midpoint")
    c2 = a.integrated_gradients(m, x, tgt, full, steps=3, rule="midpoint")
    assert torch.equal(c1.maps, c2.maps) and torch.equal(c1.total, c2.total) and torch.equal(c1.score_baseline, c2.score_baseline)
    # SmoothGrad: noise_level 0 is saliency; squared maps are non-negative; seed=None draws a seed: two calls differ
    s0, sal = a.smoothgrad(m, x, tgt, noise_level=0.0, samples=1), a.saliency(m, x, tgt)
    assert torch.equal(s0.maps, sal.maps) and torch.equal(s0.total, sal.total)
    sq = a.smoothgrad(m, x, tgt, samples=2, squared=True, seed=3)
    assert bool((sq.maps >= 0).all())
    d1, d2 = a.smoothgrad(m, x, tgt, samples=2), a.smoothgrad(m, x, tgt, samples=2)
    assert not torch.equal(d1.maps, d2.maps)
    ti = a.saliency(m, x, tgt, times_input=True, return_pixels=True)
    g = a.saliency(m, x, tgt, return_pixels=True)
    assert ti.pixels.shape == g.pixels.shape and not torch.equal(ti.pixels, g.pixels)


@pytest.mark.gpu
def test_saliency_is_the_pooled_autograd_gradient_of_the_frozen_model():
    """Within the finish gate (no times_input): pixels (C - 1) 2^-24 sum_c |g_c|, patches 8 more roundings over the patch."""
    a = _a()
    m, _ = build(img_size=64)
    for p in m.parameters():
        p.requires_grad = False
    m.eval()
    img = rng_tensor(71, (3, 3, 64, 64))
    tgt = torch.tensor([1, 2, 0])
    x = img.to(DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(m(x).gather(1, tgt.to(DEV).view(-1, 1)).sum(), x)
    res = a.saliency(m, img.to(DEV), tgt, return_pixels=True).cpu()
    px, pt, tot, mag_px, mag_pt = R.ref_finish(g.cpu().numpy())
    g_px, g_pt = R.gate_finish(3, False, mag_px, mag_pt)
    assert _violations(res.pixels.numpy(), px, g_px) == 0 and _violations(res.maps.numpy(), pt, g_pt) == 0
    exact, mag = R.exact_total(g.cpu().numpy())
    assert (np.abs(res.total.numpy() - exact) <= R.SUM_TOL * mag).all()


def prof_counts(fn):
    """Launches per kernel class (include/mfvit.h, mfvit_prof_*) of what fn() enqueues."""
    import ctypes
    lib = _L().lib()
    out = (ctypes.c_double * 40)()
    torch.cuda.synchronize()
    lib.mfvit_prof_collect(out, 10)
    lib.mfvit_prof_enable((1 << 10) - 1)
    try:
        fn()
        torch.cuda.synchronize()
        lib.mfvit_prof_collect(out, 10)
    finally:
        lib.mfvit_prof_enable(0)
    return [int(out[c * 4]) for c in range(10)]


@pytest.mark.gpu
def test_a_trainable_model_in_training_mode_is_left_as_it_was():
    a = _a()
    m, _ = build(img_size=64, drop_path_rate=0.1)
    m.train()
    assert all(p.requires_grad for n, p in m.named_parameters() if n != "pos_embed")
    img = rng_tensor(81, (3, 3, 64, 64)).to(DEV)
    tgt = torch.tensor([0, 1, 2])
    y = tgt.to(DEV)

    def calls():
        return [a.integrated_gradients(m, img, tgt, steps=2), a.smoothgrad(m, img, tgt, samples=2, seed=9), a.saliency(m, img, tgt)]
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    first = calls()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters()) and getattr(m, "_grad_arena", None) is None       # no gradient arena appeared
    assert m.training and all(mod.training for mod in m.modules()) and m._feat_cache is None
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    for r, s in zip(first, calls()):
        assert torch.equal(r.maps, s.maps) and torch.equal(r.total, s.total)
    counts = prof_counts(lambda: a.integrated_gradients(m, img, tgt, steps=2))
    assert counts[PROF_GEMM_TN] == 0 and sum(counts) > 0, counts

    def train_step():
        m.zero_grad(set_to_none=True)
        torch.manual_seed(13)
        torch.nn.functional.cross_entropy(m(img), y).backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in m.parameters() if p.grad is not None]
    before = train_step()
    m.zero_grad(set_to_none=True)
    arena = m._grad_arena
    calls()
    assert m._grad_arena is arena and all(p.grad is None for p in m.parameters())
    after = train_step()
    assert len(before) == len(after) > 20 and all(torch.equal(u, v) for u, v in zip(before, after))
    assert prof_counts(train_step)[PROF_GEMM_TN] > 0                              # (the observable does see a training step's weight gradients)


# ------------------------------------------------------------------------------------------------ 4. Fus_CrossViT
@pytest.fixture(scope="module")
def pair():
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    vit_p = [ref_vit.seeded_params(17 + i, num_classes=3, depth=2) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(19)
    backs = []
    for p in vit_p:
        b = vits.vit_small(num_classes=3, depth=2)
        b.load_state_dict(p)
        backs.append(b.to(DEV))
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    B = 2
    xc, xe = rng_tensor(93, (B, 3, 224, 224)), rng_tensor(94, (B, 3, 224, 224))
    fpd = {k: v.double() for k, v in fus_p.items()}
    vpd = [{k: v.double() for k, v in p.items()} for p in vit_p]

    def logits(a, b):
        fused, x_c, x_e = ref_fusion.fus_forward(fpd, vpd[0], vpd[1], a, b)
        return fused + x_c + x_e
    return model.to(DEV), backs, xc, xe, logits


FUS_STEPS = 4


@pytest.mark.gpu
@pytest.mark.parametrize("streams", ["both", "cxr", "enh"])
def test_fus_crossvit_integrated_gradients_match_the_float64_restatement(pair, streams):
    model, backs, xc, xe, logits = pair
    B = 2
    tgt = torch.tensor([1, 2])
    f = _oracle(logits, tgt)
    al, w = (_f32_table(v) for v in R.path_points(FUS_STEPS, "trapezoid"))
    c64, e64 = xc.double().numpy(), xe.double().numpy()
    bc = np.array([0.1, -0.2, 0.3], np.float32)
    bc64 = R._base_like(bc, c64).astype(np.float64)
    acc = [np.zeros_like(c64), np.zeros_like(e64)]
    for a_, w_ in zip(al, w):
        pc = bc64 + a_ * (c64 - bc64) if streams != "enh" else c64
        pe = a_ * e64 if streams != "cxr" else e64
        _, (gc, ge) = f(pc, pe)
        acc[0] += w_ * gc
        acc[1] += w_ * ge
    attr = [(c64 - bc64) * acc[0] if streams != "enh" else None, e64 * acc[1] if streams != "cxr" else None]
    s1 = f(c64, e64)[0]
    s0 = f(bc64 if streams != "enh" else c64, np.zeros_like(e64) if streams != "cxr" else e64)[0]
    seen = []
    if streams == "cxr":                                                          # every ENH batch the encoder is given is the input itself
        prep = backs[1]._prep_img
        backs[1]._prep_img = lambda t: (seen.append(t.detach().clone()), prep(t))[1]
    try:
        (rc, re_), share = model.integrated_gradients(backs[0], backs[1], xc.to(DEV), xe.to(DEV), tgt, baselines=(bc.tolist(), None),
                                                      streams=streams, steps=FUS_STEPS, return_pixels=True)
        (rc2, re2), share2 = model.integrated_gradients(backs[0], backs[1], xc.to(DEV), xe.to(DEV), tgt, baselines=(bc.tolist(), None),
                                                        streams=streams, steps=FUS_STEPS, return_pixels=True)
    finally:
        if streams == "cxr":
            del backs[1]._prep_img
    assert (rc is None) == (streams == "enh") and (re_ is None) == (streams == "cxr")
    worst, joint, joint_ref, mag = 0.0, 0.0, 0.0, 0.0
    for name, res, res2, at in (("cxr", rc, rc2, attr[0]), ("enh", re_, re2, attr[1])):
        if res is None:
            continue
        assert torch.equal(res.maps, res2.maps) and torch.equal(res.total, res2.total)
        e = _errors(res, (_pool(at), s1, s0), own_delta=streams != "both")
        print(f"[fus {streams} {name}] " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
        worst = max(worst, max(e.values()))
        joint, joint_ref, mag = joint + res.total.cpu().numpy(), joint_ref + at.sum(axis=(1, 2, 3)), mag + np.abs(at).sum(axis=(1, 2, 3))
    ej = float((np.abs(joint - joint_ref) / mag).max())
    print(f"[fus {streams}] joint total {ej:.2e}, worst {max(worst, ej):.2e} (gate {TOL['bf16x3']:.0e}); share {share.tolist()}")
    assert max(worst, ej) < TOL["bf16x3"]
    first = rc if rc is not None else re_
    tc = rc.total if rc is not None else torch.zeros_like(first.total)
    assert share.dtype == torch.float64 and share.shape == (B,) and share.is_cuda
    assert torch.equal(share, tc / (tc + (re_.total if re_ is not None else 0)))
    assert torch.equal(first.delta.cpu(), torch.from_numpy(joint) - (first.score_input - first.score_baseline).cpu()) and torch.equal(share, share2)
    if streams == "cxr":
        assert len(seen) >= 2 * (FUS_STEPS + 1) and all(torch.equal(t, xe.to(DEV)) for t in seen)      # (two calls)
    assert all(q.grad is None for v in backs for q in v.parameters()) and all(q.grad is None for q in model.parameters())
    assert model.training and all(v.training for v in backs)


@pytest.mark.gpu
def test_fus_crossvit_smoothgrad_saliency_and_wrong_pairs(pair):
    model, backs, xc, xe, _ = pair
    args = (backs[0], backs[1], xc.to(DEV), xe.to(DEV))
    (sc, se), share = model.saliency(*args, target=1)
    assert sc.maps.shape == se.maps.shape == (2, 14, 14) and sc.score_input is None and share.shape == (2,)
    (gc, ge), _ = model.smoothgrad(*args, target=1, samples=2, seed=5)
    (hc, he), _ = model.smoothgrad(*args, target=1, samples=2, seed=5)
    assert torch.equal(gc.maps, hc.maps) and torch.equal(ge.maps, he.maps) and not torch.equal(gc.maps, sc.maps)
    (zc, ze), _ = model.smoothgrad(*args, target=1, samples=1, noise_level=0.0)
    assert torch.equal(zc.maps, sc.maps) and torch.equal(ze.maps, se.maps)
    (oc, oe), sh = model.saliency(*args, target=1, streams="enh")
    assert oc is None and torch.equal(oe.maps, se.maps) and bool((sh == 0).all())
    import vits_returnftrs as vits
    other = vits.vit_small(num_classes=3, depth=2).to(DEV)
    for bad in ((backs[0], other, args[2], args[3]), (backs[1], backs[0], args[2], args[3]), (backs[0], backs[1], args[2], args[3][:1])):
        with pytest.raises(ValueError):
            model.integrated_gradients(*bad)


# ------------------------------------------------------------------------------------------------ 5. the maps feed the perturbation test
@pytest.mark.gpu
def test_maps_go_straight_into_the_perturbation_tests(pair):
    from mfvit import perturb
    a = _a()
    m, _ = build(img_size=64)
    x = rng_tensor(97, (3, 3, 64, 64)).to(DEV)
    res = a.integrated_gradients(m, x, 1, steps=2)
    meter = perturb.perturbation_test(m, x, res.maps, target=1, fractions=(0, .5, 1))
    out = meter.compute()
    assert out.n == 3 and len(out.mean_prob) == 3 and all(math.isfinite(v) for v in out.mean_prob)
    model, backs, xc, xe, _ = pair
    (rc, re_), _ = model.saliency(backs[0], backs[1], xc.to(DEV), xe.to(DEV), target=2, sign="abs")
    fm = model.perturbation_test(backs[0], backs[1], xc.to(DEV), xe.to(DEV), maps=(rc.maps, re_.maps), target=2, fractions=(0, .5))
    assert fm.compute().n == 2
