"""Gradient attribution (include/mfvit.h: mfvit_attr_inputs, mfvit_attr_accumulate, mfvit_attr_finish; mfvit.attribution): the float64
restatements of tests/attribution_ref.py pinned on closed forms, the noise hash, the gates of the three kernels (derived in attribution_ref's
docstring from the kernels' operation orders) shown to pass the kernels' arithmetic and to catch planted bugs, and the argument contract - no
GPU needed.

Every C call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import attribution_ref as R
from mfvit import attribution as A          # (at module level: without the feature every test here fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
EINVAL = -22
FAKE = 1 << 30


def _lib():
    from mfvit import _lib
    return _lib


def _attr():
    return A


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------------------------------------------- the quadrature
@pytest.mark.parametrize("rule", ["trapezoid", "midpoint"])
@pytest.mark.parametrize("steps", [1, 2, 7, 20, 64])
def test_path_table_weights_sum_to_one(steps, rule):
    al, w = _attr().path_table(steps, rule)
    assert len(al) == len(w) == (steps + 1 if rule == "trapezoid" else steps)
    assert abs(math.fsum(w) - 1.0) <= 1e-15
    assert all(0.0 <= a <= 1.0 for a in al) and al == sorted(al)
    assert (al[0], al[-1]) == ((0.0, 1.0) if rule == "trapezoid" else (0.5 / steps, (steps - 0.5) / steps))
    assert (al, w) == R.path_points(steps, rule)                                 # the restatement walks the same path


def _linear(wt):
    return lambda p: ((p * wt).sum(axis=(1, 2, 3)), np.broadcast_to(wt, p.shape).copy())


def _quadratic(wt):
    # score = sum w p^2 / 2: its gradient is linear in alpha, which both rules integrate exactly
    return lambda p: ((wt * p * p).sum(axis=(1, 2, 3)) / 2, wt * p)


def _smooth(wt):
    return lambda p: (np.tanh((wt * p).sum(axis=(1, 2, 3))), (1 - np.tanh((wt * p).sum(axis=(1, 2, 3))) ** 2).reshape(-1, 1, 1, 1) * wt)


@pytest.mark.parametrize("rule", ["trapezoid", "midpoint"])
@pytest.mark.parametrize("steps", [1, 3, 8])
def test_linear_and_quadratic_scores_are_integrated_exactly(steps, rule):
    g = _rng(steps)
    x, x0, wt = (g.standard_normal((2, 3, 4, 4)) for _ in range(3))
    al, w = R.path_points(steps, rule)
    attr, s1, s0 = R.integrated_gradients(_linear(wt), x, x0, al, w)
    assert np.abs(attr - (x - x0) * wt).max() <= 1e-12
    assert np.abs(attr.sum(axis=(1, 2, 3)) - (s1 - s0)).max() <= 1e-12
    attr, s1, s0 = R.integrated_gradients(_quadratic(wt), x, x0, al, w)
    assert np.abs(attr - (x - x0) * wt * (x + x0) / 2).max() <= 1e-12
    assert np.abs(attr.sum(axis=(1, 2, 3)) - (s1 - s0)).max() <= 1e-12


@pytest.mark.parametrize("rule", ["trapezoid", "midpoint"])
def test_completeness_gap_of_a_smooth_score_falls_fourfold_per_doubling(rule):
    g = _rng(5)
    x, x0 = g.standard_normal((3, 3, 4, 4)), np.zeros((3, 3, 4, 4))
    wt = g.standard_normal((3, 3, 4, 4)) * 0.2
    gaps = []
    for steps in (4, 8, 16, 32):
        al, w = R.path_points(steps, rule)
        attr, s1, s0 = R.integrated_gradients(_smooth(wt), x, x0, al, w)
        gaps.append(np.abs(attr.sum(axis=(1, 2, 3)) - (s1 - s0)))
    for a, b in zip(gaps, gaps[1:]):
        print(f"[{rule}] |delta| {a.max():.3e} -> {b.max():.3e}")
        assert (b < a / 3).all(), (a, b)


def test_smoothgrad_without_noise_is_saliency():
    g = _rng(6)
    x, wt = g.standard_normal((2, 3, 4, 4)), g.standard_normal((2, 3, 4, 4))
    f = _smooth(wt)
    assert np.array_equal(R.smoothgrad(f, x, [np.zeros_like(x)]), f(x)[1])
    sq = R.smoothgrad(f, x, [np.zeros_like(x)] * 4, squared=True)
    assert np.abs(sq - f(x)[1] ** 2).max() <= 1e-15 * np.abs(sq).max()


# ------------------------------------------------------------------------------------------------------- the noise hash
def test_hash_words_are_the_published_functions():
    assert int(R.lowbias32(0)) == 0 and int(R.lowbias32b(0)) == 0                # both fix 0 (xorshift-multiply)
    def scalar(x, m1, m2, last):
        x ^= x >> 16; x = x * m1 & 0xFFFFFFFF; x ^= x >> 15; x = x * m2 & 0xFFFFFFFF; x ^= x >> last
        return x
    for v in (1, 2, 0x9E3779B9, 0xFFFFFFFF, 123456789):
        assert int(R.lowbias32(v)) == scalar(v, 0x7feb352d, 0x846ca68b, 16) and int(R.lowbias32b(v)) == scalar(v, 0x21f0aaad, 0x735a2d97, 15)
    x = np.arange(1 << 16, dtype=np.uint64)
    assert len(np.unique(R.lowbias32(x))) == len(x) and len(np.unique(R.lowbias32b(x))) == len(x)     # bijections
    assert not np.array_equal(R.lowbias32(x), R.lowbias32b(x))


def test_u1_is_never_zero_and_u2_stays_below_one():
    # the extreme words: h >> 8 == 0 and h >> 8 == 2^24 - 1
    lo = (np.float32(0) + np.float32(0.5)) * np.float32(2.0 ** -24)
    hi = (np.float32(2 ** 24 - 1) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert lo == 2.0 ** -25 and hi == 1.0                                        # (2^24 - 1/2 rounds to 2^24 in f32: u1 = 1, z = 0)
    assert np.float32(2 ** 24 - 1) * np.float32(2.0 ** -24) < 1.0
    u1, u2 = R.uniforms(123, 0, 0, 1 << 18)
    assert u1.dtype == u2.dtype == np.float32 and u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert np.isfinite(R.ref_normal(123, 0, 0, 1 << 18)).all()


def test_noise_depends_on_the_global_sample_index_only():
    shape = (2, 3, 16, 16)
    whole = R.ref_noise(77, 0, 4, shape)
    assert np.array_equal(whole[2:], R.ref_noise(77, 2, 2, shape))                # grouping: [0, 4) = [0, 2) + [2, 4)
    assert np.array_equal(whole[:2], R.ref_noise(77, 0, 2, shape))
    flat = whole.reshape(4, 2, -1)
    assert len({flat[s, b].tobytes() for s in range(4) for b in range(2)}) == 8   # every (sample, image) its own stream
    assert not np.array_equal(whole, R.ref_noise(78, 0, 4, shape))
    assert not np.array_equal(R.ref_noise(77 + (1 << 32), 0, 1, shape), whole[:1])                  # the high word of the seed counts


def test_noise_moments_of_a_million_draws():
    n = 1_000_000
    z = R.ref_normal(2024, 3, 1, n)
    mean, var = z.mean(), z.var()
    print(f"[moments] mean {mean:.3e} (bound {5 / math.sqrt(n):.3e}), var - 1 {var - 1:.3e} (bound {5 * math.sqrt(2 / n):.3e})")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(np.mean(z ** 3)) <= 5 * math.sqrt(15 / n) and abs(np.mean(z ** 4) - 3) <= 5 * math.sqrt(96 / n)


# ------------------------------------------------------------------------------------------------------- the gates
SHAPES = [(2, 3, 16, 16), (3, 3, 32, 48), (2, 1, 48, 32)]
ALPHA = np.array([0.0, 1.0, 0.5, 1.0 / 3.0], dtype=np.float32)


def _case(shape, seed, full):
    g = _rng(seed)
    x = g.standard_normal(shape).astype(np.float32)
    base = (g.standard_normal(shape) if full else (0.5 + np.arange(shape[1])) * -1.25).astype(np.float32)
    return x, base


def _violations(got, ref, gate):
    return int((np.abs(got.astype(np.float64) - ref) > gate).sum())


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_inputs_gate_passes_the_kernels_arithmetic_and_catches_a_skipped_group(shape, full):
    """Gate (attribution_ref): |v - ref| <= U (|alpha (x - base)| + |ref|), end points exact."""
    x, base = _case(shape, sum(shape), full)
    ref = R.ref_inputs(x, base, ALPHA)
    gate = R.gate_inputs(x, base, ALPHA, ref)
    got = R.mirror_inputs(x, base, ALPHA)
    assert _violations(got, ref, gate) == 0
    assert np.array_equal(got[0], R._base_like(base, x).astype(np.float32)) and np.array_equal(got[1], x)
    assert _violations(R.mirror_inputs(x, base, ALPHA, mutate="skip_second_group"), ref, gate) > 0
    one_ulp = got.copy()
    one_ulp[2] = np.nextafter(np.nextafter(got[2], np.float32(np.inf)), np.float32(np.inf))
    assert _violations(one_ulp, ref, gate) > 0                                  # two ulp off: caught


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_accumulate_gate_passes_the_kernels_arithmetic_and_catches_a_dropped_step(shape, k, power):
    """Gate (attribution_ref): k U sum_s |w_s g^p|."""
    g = _rng(sum(shape) + k)
    grad = g.standard_normal((k,) + shape).astype(np.float32)
    w = (g.random(k) + 0.1).astype(np.float32)
    ref, gate = R.ref_accumulate(grad, w, power), R.gate_accumulate(grad, w, power)
    assert _violations(R.mirror_accumulate(grad, w, power), ref, gate) == 0
    assert _violations(R.mirror_accumulate(grad, w, power, mutate="drop_last_step"), ref, gate) > 0
    assert _violations(R.mirror_accumulate(grad, w, power, mutate="skip_second_group"), ref, gate) > 0


@pytest.mark.parametrize("absval", [False, True])
@pytest.mark.parametrize("times_input", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_finish_gates_pass_the_kernels_tree_and_catch_dropped_terms(shape, times_input, absval):
    """Gates (attribution_ref): pixels (2 + C - 1) U sum_c |t_c|, patches 8 U more over the patch (2 only with times_input), total 1e-12 sum |t|."""
    g = _rng(sum(shape) + 7)
    acc = g.standard_normal(shape).astype(np.float32)
    x, base = _case(shape, sum(shape) + 8, True)
    args = (acc, x, base) if times_input else (acc,)
    px, pt, tot, mag_px, mag_pt = R.ref_finish(*args, absval=absval)
    g_px, g_pt = R.gate_finish(shape[1], times_input, mag_px, mag_pt)
    exact, mag = R.exact_total(R.f32_terms(*args))

    def bad(mutate):
        m_px, m_pt, m_tot = R.mirror_finish(*args, absval=absval, mutate=mutate)
        return _violations(m_px, px, g_px), _violations(m_pt, pt, g_pt), int((np.abs(m_tot - exact) > R.SUM_TOL * mag).sum())
    assert bad(None) == (0, 0, 0)
    assert abs(tot - exact).max() <= 2 * R.U * R.SLACK * mag.max()                  # the f32 terms against the float64 ones
    if shape[1] > 1:
        assert bad("drop_channel")[0] > 0 and bad("drop_channel")[1] > 0
    assert bad("drop_row")[1] > 0 and bad("drop_col")[1] > 0
    assert bad("f32_total")[2] > 0


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_lib_binds_the_entry_points():
    L = _lib()
    h = L.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mfvit.h")).read(), flags=re.S)
    for name, arity in (("mfvit_attr_inputs", 13), ("mfvit_attr_accumulate", 8), ("mfvit_attr_finish", 14)):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/mfvit.h"
        assert name in L.SIGNATURES and hasattr(h, name)
        assert len(L.SIGNATURES[name][1]) == arity
        assert len(re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")) == arity
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5                          # additive: the version stays


B_, C_, HW_, S_ = 2, 3, 32 * 48, 4
IMG_BYTES = B_ * C_ * HW_ * 4
X, OUT, BASE, ALPHAP, SIGMA, SEED = FAKE, FAKE + 2 * IMG_BYTES, FAKE + 16 * IMG_BYTES, FAKE + 32 * IMG_BYTES, FAKE + 33 * IMG_BYTES, FAKE + 34 * IMG_BYTES
# (x, base, base_full, alpha, sigma, seed, s0, out, S, B, C, hw)
INPUTS_INVALID = {
    "x_null": (None, BASE, 0, ALPHAP, None, None, 0, OUT, S_, B_, C_, HW_),
    "base_null": (X, None, 0, ALPHAP, None, None, 0, OUT, S_, B_, C_, HW_),
    "alpha_null": (X, BASE, 0, None, None, None, 0, OUT, S_, B_, C_, HW_),
    "out_null": (X, BASE, 0, ALPHAP, None, None, 0, None, S_, B_, C_, HW_),
    "sigma_without_seed": (X, BASE, 0, ALPHAP, SIGMA, None, 0, OUT, S_, B_, C_, HW_),
    "S_zero": (X, BASE, 0, ALPHAP, None, None, 0, OUT, 0, B_, C_, HW_),
    "S_65536": (X, BASE, 0, ALPHAP, None, None, 0, FAKE + (1 << 40), 65536, 1, 1, 16),
    "B_zero": (X, BASE, 0, ALPHAP, None, None, 0, OUT, S_, 0, C_, HW_),
    "B_65536": (X, BASE, 0, ALPHAP, None, None, 0, FAKE + (1 << 40), 1, 65536, 1, 16),
    "C_negative": (X, BASE, 0, ALPHAP, None, None, 0, OUT, S_, B_, -3, HW_),
    "hw_zero": (X, BASE, 0, ALPHAP, None, None, 0, OUT, S_, B_, C_, 0),
    "s0_negative": (X, BASE, 0, ALPHAP, SIGMA, SEED, -1, OUT, S_, B_, C_, HW_),
    "CHW_above_2_30": (X, BASE, 0, ALPHAP, None, None, 0, FAKE + (1 << 40), 1, 1, 4100, 512 * 512),
    "out_is_x": (X, BASE, 0, ALPHAP, None, None, 0, X, S_, B_, C_, HW_),
    "out_overlaps_x_tail": (X, BASE, 0, ALPHAP, None, None, 0, X + IMG_BYTES - 16, S_, B_, C_, HW_),
    "out_ends_inside_full_base": (X, OUT + S_ * IMG_BYTES - 16, 1, ALPHAP, None, None, 0, OUT, S_, B_, C_, HW_),
}


@pytest.mark.parametrize("case", sorted(INPUTS_INVALID))
def test_attr_inputs_refuses_invalid_calls_without_a_device(case):
    assert _lib().lib().mfvit_attr_inputs(*INPUTS_INVALID[case], None) == EINVAL


# (g, w, acc, k, B, n, power)
ACC_INVALID = {
    "g_null": (None, ALPHAP, X, 3, B_, C_ * HW_, 1),
    "w_null": (OUT, None, X, 3, B_, C_ * HW_, 1),
    "acc_null": (OUT, ALPHAP, None, 3, B_, C_ * HW_, 1),
    "k_zero": (OUT, ALPHAP, X, 0, B_, C_ * HW_, 1),
    "B_zero": (OUT, ALPHAP, X, 3, 0, C_ * HW_, 1),
    "B_65536": (FAKE + (1 << 40), ALPHAP, X, 1, 65536, 16, 1),
    "n_zero": (OUT, ALPHAP, X, 3, B_, 0, 1),
    "n_above_2_30": (FAKE + (1 << 40), ALPHAP, X, 1, 1, (1 << 30) + 4, 1),
    "power_zero": (OUT, ALPHAP, X, 3, B_, C_ * HW_, 0),
    "power_three": (OUT, ALPHAP, X, 3, B_, C_ * HW_, 3),
    "acc_inside_g": (OUT, ALPHAP, OUT + IMG_BYTES, 3, B_, C_ * HW_, 1),
}


@pytest.mark.parametrize("case", sorted(ACC_INVALID))
def test_attr_accumulate_refuses_invalid_calls_without_a_device(case):
    assert _lib().lib().mfvit_attr_accumulate(*ACC_INVALID[case], None) == EINVAL


PIX, PAT, TOT = FAKE + 40 * IMG_BYTES, FAKE + 48 * IMG_BYTES, FAKE + 49 * IMG_BYTES
# (acc, x, base, base_full, times_input, absval, pixels, patches, total, B, C, H, W)
FINISH_INVALID = {
    "acc_null": (None, X, BASE, 0, 1, 0, PIX, PAT, TOT, B_, C_, 32, 48),
    "patches_null": (OUT, X, BASE, 0, 1, 0, PIX, None, TOT, B_, C_, 32, 48),
    "total_null": (OUT, X, BASE, 0, 1, 0, PIX, PAT, None, B_, C_, 32, 48),
    "times_input_without_x": (OUT, None, BASE, 0, 1, 0, PIX, PAT, TOT, B_, C_, 32, 48),
    "times_input_without_base": (OUT, X, None, 0, 1, 0, PIX, PAT, TOT, B_, C_, 32, 48),
    "H_not_multiple_of_16": (OUT, X, BASE, 0, 1, 0, PIX, PAT, TOT, B_, C_, 40, 48),
    "W_not_multiple_of_16": (OUT, X, BASE, 0, 1, 0, PIX, PAT, TOT, B_, C_, 32, 56),
    "H_zero": (OUT, X, BASE, 0, 1, 0, PIX, PAT, TOT, B_, C_, 0, 48),
    "B_zero": (OUT, X, BASE, 0, 1, 0, PIX, PAT, TOT, 0, C_, 32, 48),
    "C_zero": (OUT, X, BASE, 0, 1, 0, PIX, PAT, TOT, B_, 0, 32, 48),
    "CHW_above_2_30": (OUT, X, BASE, 0, 1, 0, PIX, PAT, TOT, 1, 4100, 512, 512),
    "pixels_is_acc": (OUT, X, BASE, 0, 0, 0, OUT, PAT, TOT, B_, C_, 32, 48),
    "pixels_inside_x": (OUT, X, BASE, 0, 1, 0, X + 64, PAT, TOT, B_, C_, 32, 48),
}


@pytest.mark.parametrize("case", sorted(FINISH_INVALID))
def test_attr_finish_refuses_invalid_calls_without_a_device(case):
    assert _lib().lib().mfvit_attr_finish(*FINISH_INVALID[case], None) == EINVAL


# ------------------------------------------------------------------------------------------------------- argument errors of the Python layer
def _small_vit():
    import vits
    return vits.vit_small(num_classes=3, depth=1, img_size=32)


def test_argument_errors_come_before_any_launch_and_cpu_tensors_are_refused():
    a = _attr()
    MfvitError = _lib().MfvitError
    m = _small_vit()
    img = torch.zeros(2, 3, 32, 32)
    for kw in (dict(steps=0), dict(steps=-3), dict(steps=2.5), dict(rule="simpson"), dict(score="margin"), dict(sign="positive"),
               dict(baseline=[0.1, 0.2]), dict(baseline=torch.zeros(2, 3, 32, 16)), dict(baseline=torch.zeros(4)), dict(max_batch=1),
               dict(target=3), dict(target=-1), dict(target=torch.zeros(3, dtype=torch.int64)), dict(target=1.5), dict(noise=-0.1)):
        with pytest.raises(ValueError):
            a.integrated_gradients(m, img, **kw)
    for kw in (dict(noise_level=-0.5), dict(noise_level=float("nan")), dict(samples=0), dict(samples=1.5), dict(seed=-1), dict(seed=0.5),
               dict(score="x"), dict(sign="x"), dict(max_batch=1)):
        with pytest.raises(ValueError):
            a.smoothgrad(m, img, **kw)
    for bad in (torch.zeros(3, 32, 32), torch.zeros(2, 3, 30, 32), torch.zeros(0, 3, 32, 32), [[1.0]]):
        with pytest.raises(ValueError):
            a.saliency(m, bad)
    # valid arguments, CPU tensors: loud failure, no fallback
    for call in (lambda: a.integrated_gradients(m, img, target=1, baseline=[0.1, 0.2, 0.3], steps=2),
                 lambda: a.integrated_gradients(m, img, baseline=torch.zeros(2, 3, 32, 32)),
                 lambda: a.smoothgrad(m, img, target=torch.tensor([0, 2]), samples=2, seed=5),
                 lambda: a.saliency(m, img, times_input=True, sign="abs", score="prob")):
        with pytest.raises(MfvitError):
            call()
    assert all(p.grad is None for p in m.parameters())


def test_fus_crossvit_argument_errors():
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    backs = [vits.vit_small(num_classes=3, depth=1) for _ in range(2)]
    model = fus.Fus_CrossViT(backs[0], backs[1])
    xc, xe = torch.zeros(2, 3, 224, 224), torch.zeros(2, 3, 224, 224)
    other = vits.vit_small(num_classes=3, depth=1)
    for args in ((backs[0], other, xc, xe), (backs[1], backs[0], xc, xe), (backs[0], backs[1], xc, xe[:1])):      # _check_pair
        with pytest.raises(ValueError):
            model.integrated_gradients(*args)
    for kw in (dict(streams="left"), dict(baselines=None), dict(baselines=(None,)), dict(baselines=([1.0, 2.0], None)), dict(steps=0),
               dict(rule="x"), dict(target=3)):
        with pytest.raises(ValueError):
            model.integrated_gradients(backs[0], backs[1], xc, xe, **kw)
    with pytest.raises(ValueError):
        model.smoothgrad(backs[0], backs[1], xc, xe, samples=0)
    with pytest.raises(ValueError):
        model.saliency(backs[0], backs[1], xc, xe, streams="none")
    for call in (lambda: model.integrated_gradients(backs[0], backs[1], xc, xe, steps=2),
                 lambda: model.smoothgrad(backs[0], backs[1], xc, xe, samples=2, seed=1, streams="cxr"),
                 lambda: model.saliency(backs[0], backs[1], xc, xe, streams="enh")):
        with pytest.raises(_lib().MfvitError):
            call()


def test_result_cpu_on_host_tensors_is_the_identity_and_keeps_dtypes():
    a = _attr()
    r = a.AttributionResult(torch.zeros(2, 2, 2), None, torch.zeros(2, dtype=torch.float64))
    assert r.cpu() is r and "maps=(2, 2, 2)" in repr(r) and "pixels" not in repr(r)
