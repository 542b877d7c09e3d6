"""Mixup / CutMix / random erasing and the soft-target cross entropy (include/mfvit.h: mfvit_batch_mix, mfvit_cross_entropy_soft;
mfvit.mixup, mfvit.losses.soft_cross_entropy): the host-side contract, no GPU needed.

Every C call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FAKE = 1 << 30          # non-NULL pointer values the argument checks accept (nothing is ever read from them)
N, C, H, W = 4, 3, 8, 8
BYTES = N * C * H * W * 4
A, B_, OA, OB, DESC, LAM = FAKE, FAKE + 2 * BYTES, FAKE + 4 * BYTES, FAKE + 6 * BYTES, FAKE + 8 * BYTES, FAKE + 9 * BYTES


def _lib():
    from mfvit import _lib
    return _lib


def _mixup(**kw):
    from mfvit.mixup import Mixup
    return Mixup(**kw)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_header_declares_and_lib_binds_the_entry_points():
    L = _lib()
    h = L.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mfvit.h")).read(), flags=re.S)
    for name in ("mfvit_batch_mix", "mfvit_cross_entropy_soft"):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/mfvit.h"
        assert name in L.SIGNATURES and hasattr(h, name)
    assert len(L.SIGNATURES["mfvit_batch_mix"][1]) == 11 and len(L.SIGNATURES["mfvit_cross_entropy_soft"][1]) == 11
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5


BATCH_MIX_INVALID = {
    "out_a_is_a": (A, None, A, None, N, C, H, W),
    "out_b_is_b": (A, B_, OA, B_, N, C, H, W),
    "out_a_overlaps_a_tail": (A, None, A + BYTES - 16, None, N, C, H, W),
    "out_a_overlaps_a_head": (A + 64, None, A, None, N, C, H, W),
    "out_a_overlaps_b": (A, B_, B_ + 16, OB, N, C, H, W),
    "out_b_overlaps_a": (A, B_, OA, A + BYTES // 2, N, C, H, W),
    "out_a_overlaps_out_b": (A, B_, OA, OA + BYTES - 4, N, C, H, W),
    "b_without_out_b": (A, B_, OA, None, N, C, H, W),
    "out_b_without_b": (A, None, OA, OB, N, C, H, W),
    "n_zero": (A, None, OA, None, 0, C, H, W),
    "n_negative": (A, None, OA, None, -1, C, H, W),
    "C_zero": (A, None, OA, None, N, 0, H, W),
    "H_zero": (A, None, OA, None, N, C, 0, W),
    "W_negative": (A, None, OA, None, N, C, H, -8),
}


@pytest.mark.parametrize("case", sorted(BATCH_MIX_INVALID))
def test_batch_mix_refuses_invalid_calls_without_a_device(case):
    a, b, oa, ob, n, c, h, w = BATCH_MIX_INVALID[case]
    assert _lib().lib().mfvit_batch_mix(a, b, oa, ob, DESC, LAM, n, c, h, w, None) == EINVAL


CE_SOFT_INVALID = {
    "partner_without_lam": (FAKE, None, 0.1, 4, 3),
    "lam_without_partner": (None, FAKE, 0.1, 4, 3),
    "C_65": (None, None, 0.0, 4, 65),
    "C_zero": (None, None, 0.0, 4, 0),
    "B_zero": (None, None, 0.0, 0, 3),
    "smoothing_one": (None, None, 1.0, 4, 3),
    "smoothing_negative": (None, None, -0.01, 4, 3),
    "smoothing_nan": (None, None, float("nan"), 4, 3),
}


@pytest.mark.parametrize("case", sorted(CE_SOFT_INVALID))
def test_cross_entropy_soft_refuses_invalid_calls_without_a_device(case):
    partner, lam, smoothing, b, c = CE_SOFT_INVALID[case]
    h = _lib().lib()
    assert h.mfvit_cross_entropy_soft(FAKE, FAKE, partner, lam, smoothing, FAKE, FAKE, FAKE, b, c, None) == EINVAL


# ------------------------------------------------------------------------------------------------------- sample_params
@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_tables_have_the_abi_shapes_and_a_seed_reproduces_them(mode):
    m = _mixup(mode=mode, erase_prob=0.5)
    d1, l1 = m.sample_params(9, 30, 34, gen(5))
    d2, l2 = m.sample_params(9, 30, 34, gen(5))
    d3, l3 = m.sample_params(9, 30, 34, gen(6))
    assert d1.shape == (9, 12) and d1.dtype == torch.int32 and not d1.is_cuda
    assert l1.shape == (9,) and l1.dtype == torch.float32 and not l1.is_cuda
    assert torch.equal(d1, d2) and torch.equal(l1, l2)
    assert not (torch.equal(d1, d3) and torch.equal(l1, l3))
    assert int(d1[:, 11].abs().max()) == 0


def test_prob_zero_mixes_nothing():
    d, l = _mixup(prob=0.0, mode="elem").sample_params(16, 32, 32, gen(1))
    assert int(d[:, 1].abs().max()) == 0 and bool((l == 1).all()) and int(d[:, 2:6].abs().max()) == 0
    d, l = _mixup(mixup_alpha=0.0, cutmix_alpha=0.0).sample_params(16, 32, 32, gen(1))
    assert int(d[:, 1].abs().max()) == 0 and bool((l == 1).all())


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_batch_mode_has_one_distinct_row_up_to_the_partner(seed):
    d, l = _mixup(mode="batch").sample_params(8, 64, 48, gen(seed))
    assert bool((d[:, 1:] == d[0, 1:]).all()) and bool((l == l[0]).all())


@pytest.mark.parametrize("n", [8, 9])
def test_pair_mode_shares_a_draw_between_both_halves(n):
    d, l = _mixup(mode="pair").sample_params(n, 64, 48, gen(11))
    for i in range(n):
        assert float(l[i]) == float(l[n - 1 - i])
        assert torch.equal(d[i, 1:6], d[n - 1 - i, 1:6])
    assert len(set(l.tolist())) > 1                      # ... and not one draw for the whole batch


@pytest.mark.parametrize("mode,partner", [("batch", "flip"), ("elem", "flip"), ("elem", "perm"), ("pair", "flip")])
@pytest.mark.parametrize("hw", [(30, 34), (224, 224), (1, 7)])
def test_boxes_lie_inside_the_image_and_lam_in_the_unit_interval(mode, partner, hw):
    from mfvit.mixup import check_params
    H_, W_ = hw
    m = _mixup(mode=mode, partner=partner, erase_prob=0.7)
    for seed in range(4):
        d, l = m.sample_params(33, H_, W_, gen(seed))
        check_params(d, l, 33, H_, W_)
        for c0 in (2, 7):
            assert bool((d[:, c0] >= 0).all()) and bool((d[:, c0] <= d[:, c0 + 1]).all()) and bool((d[:, c0 + 1] <= H_).all())
            assert bool((d[:, c0 + 2] >= 0).all()) and bool((d[:, c0 + 2] <= d[:, c0 + 3]).all()) and bool((d[:, c0 + 3] <= W_).all())
        assert bool((l >= 0).all()) and bool((l <= 1).all())
        assert set(d[:, 1].tolist()) <= {0, 1, 2} and set(d[:, 6].tolist()) <= {0, 1}


def test_corrected_lam_is_the_f32_of_the_f64_area_share():
    H_, W_ = 37, 53
    d, l = _mixup(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem", correct_lam=True).sample_params(200, H_, W_, gen(3))
    assert bool((d[:, 1] == 2).all())
    area = (d[:, 3] - d[:, 2]).double() * (d[:, 5] - d[:, 4]).double()
    assert torch.equal(l, (1.0 - area / float(H_ * W_)).float())
    assert len(set(area.tolist())) > 20
    # without the correction lam stays the Beta draw
    d2, l2 = _mixup(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem", correct_lam=False).sample_params(200, H_, W_, gen(3))
    assert torch.equal(d2, d) and not torch.equal(l2, l)


@pytest.mark.parametrize("n", [1, 2, 7, 128])
def test_partners(n):
    d, _ = _mixup(partner="flip").sample_params(n, 16, 16, gen(2))
    j = d[:, 0].long()
    assert j.tolist() == list(range(n - 1, -1, -1)) and j[j].tolist() == list(range(n))          # an involution
    d, _ = _mixup(partner="perm", mode="elem").sample_params(n, 16, 16, gen(2))
    assert sorted(d[:, 0].tolist()) == list(range(n))
    if n == 128:
        assert d[:, 0].tolist() != list(range(n - 1, -1, -1)) and d[:, 0].tolist() != list(range(n))


def test_erase_boxes_respect_the_scale_up_to_the_rounding_of_their_sides():
    H_, W_, scale, ratio = 224, 200, (0.02, 1 / 3), (0.3, 3.3)
    d, _ = _mixup(prob=0.0, erase_prob=1.0, erase_scale=scale, erase_ratio=ratio).sample_params(400, H_, W_, gen(4))
    on = d[:, 6] == 1
    assert int(on.sum()) > 300 and int(d[~on, 7:11].abs().max() if bool((~on).any()) else 0) == 0
    h = (d[on, 8] - d[on, 7]).double()
    w = (d[on, 10] - d[on, 9]).double()
    assert bool((h > 0).all()) and bool((w > 0).all()) and bool((h < H_).all()) and bool((w < W_).all())
    # h = round(sqrt(area * aspect)), w = round(sqrt(area / aspect)): each side is within 0.5 of its real value
    assert bool(((h - 0.5) * (w - 0.5) <= scale[1] * H_ * W_).all())
    assert bool(((h + 0.5) * (w + 0.5) >= scale[0] * H_ * W_).all())
    assert bool(((h + 0.5) / (w - 0.5) >= ratio[0]).all()) and bool(((h - 0.5) / (w + 0.5) <= ratio[1]).all())
    assert len(set(zip(h.tolist(), w.tolist()))) > 50
    # erase_prob = 0 draws no box, and about erase_prob of the samples get one
    d0, _ = _mixup(erase_prob=0.0).sample_params(64, H_, W_, gen(4))
    assert int(d0[:, 6:11].abs().max()) == 0
    dh, _ = _mixup(prob=0.0, erase_prob=0.25).sample_params(2000, H_, W_, gen(9))
    assert abs(float((dh[:, 6] == 1).float().mean()) - 0.25) < 4 * math.sqrt(0.25 * 0.75 / 2000)


@pytest.mark.parametrize("switch_prob", [0.5, 0.2])
def test_cutmix_share_follows_switch_prob(switch_prob):
    n = 2000
    d, _ = _mixup(mode="elem", switch_prob=switch_prob).sample_params(n, 32, 32, gen(2024))
    assert set(d[:, 1].tolist()) == {1, 2}
    share = float((d[:, 1] == 2).float().mean())
    assert abs(share - switch_prob) <= 4 * math.sqrt(switch_prob * (1 - switch_prob) / n), share


# ------------------------------------------------------------------------------------------------------- MixTarget
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("C_", [3, 64])
def test_dense_target_rows_sum_to_one_and_equal_the_float64_formula(smoothing, C_):
    from mfvit.mixup import MixTarget
    g = gen(7)
    Bn = 33
    t = torch.randint(0, C_, (Bn,), generator=g)
    p = torch.randperm(Bn, generator=g).int()
    lam = torch.rand(Bn, generator=g)
    lam[0], lam[1] = 1.0, 0.0
    y = MixTarget(t, p, lam, smoothing).dense(C_)
    assert y.shape == (Bn, C_) and y.dtype == torch.float32
    assert float((y.double().sum(1) - 1).abs().max()) <= 1e-6
    ref = torch.zeros(Bn, C_, dtype=torch.float64)
    for i in range(Bn):
        for c in range(C_):
            si = (1 - smoothing) * (c == int(t[i])) + smoothing / C_
            sj = (1 - smoothing) * (c == int(t[int(p[i])])) + smoothing / C_
            ref[i, c] = float(lam[i]) * si + (1 - float(lam[i])) * sj
    assert float((y.double() - ref).abs().max()) <= 2.0 ** -24
    hard = MixTarget(t, smoothing=smoothing).dense(C_)
    assert float((hard.double().sum(1) - 1).abs().max()) <= 1e-6
    assert hard.argmax(1).tolist() == t.tolist()
    with pytest.raises(ValueError):
        MixTarget(torch.tensor([0, C_])).dense(C_)
    with pytest.raises(ValueError):
        MixTarget(t, partner=p)


# ------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_are_raised_from_python_before_any_launch():
    from mfvit.losses import soft_cross_entropy
    from mfvit.mixup import check_params
    MfvitError = _lib().MfvitError
    m = _mixup(num_classes=3)
    x, t = torch.zeros(4, 3, 8, 8), torch.tensor([0, 1, 2, 0])
    with pytest.raises(ValueError, match="shape"):
        m(x, t, torch.zeros(4, 3, 8, 6))                         # the two streams differ
    with pytest.raises(ValueError, match="num_classes"):
        m(x, torch.tensor([0, 1, 3, 0]))
    with pytest.raises(ValueError, match="requires_grad|autograd"):
        m(x.clone().requires_grad_(True), t)
    with pytest.raises(ValueError):
        m(x, t[:3])
    d, l = m.sample_params(4, 8, 8, gen(0))
    check_params(d, l, 4, 8, 8)
    for col, val in ((0, 4), (0, -1), (1, 3), (3, 9), (2, -1), (5, 9), (8, 9), (9, -2)):
        bad = d.clone()
        bad[1, col] = val
        with pytest.raises(ValueError, match="desc out of range"):
            check_params(bad, l, 4, 8, 8)
        with pytest.raises(ValueError, match="desc out of range"):
            m(x, t, params=(bad, l))
    bad = d.clone()
    bad[0, 2], bad[0, 3] = 5, 4                                  # yl > yh
    with pytest.raises(ValueError, match="desc out of range"):
        check_params(bad, l, 4, 8, 8)
    with pytest.raises(ValueError, match="lam"):
        check_params(d, l + 1.5, 4, 8, 8)
    with pytest.raises(ValueError):
        check_params(d[:3], l, 4, 8, 8)
    with pytest.raises(MfvitError):
        m(x, t)                                                  # valid arguments, CPU tensors: loud failure, no fallback
    with pytest.raises(MfvitError):
        soft_cross_entropy(torch.zeros(4, 3), t, smoothing=0.1)
    with pytest.raises(ValueError):
        soft_cross_entropy(torch.zeros(4, 3), t, smoothing=1.0)
    with pytest.raises(ValueError):
        soft_cross_entropy(torch.zeros(4, 3), t[:3])
    for kw in (dict(mode="pixel"), dict(partner="roll"), dict(mode="pair", partner="perm"), dict(label_smoothing=1.0), dict(prob=1.5),
               dict(erase_scale=(0.5, 0.1))):
        with pytest.raises(ValueError):
            _mixup(**kw)


def test_eval_mode_and_disabled_return_the_inputs_and_a_hard_target():
    x, x2, t = torch.zeros(4, 3, 8, 8), torch.ones(4, 3, 8, 8), torch.tensor([0, 1, 2, 0])
    for m in (_mixup().eval(), _mixup(enabled=False)):
        a, b, y = m(x, t, x2)
        assert a is x and b is x2
        assert y.partner is None and y.lam is None and y.smoothing == 0.0 and torch.equal(y.target, t)
        a, y = m(x, t)
        assert a is x
