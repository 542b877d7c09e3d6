"""The perturbation test for relevance maps (include/mfvit.h: mfvit_patch_rank, mfvit_patch_perturb, mfvit_perturb_score; mfvit.perturb):
the rank rule, the host-side tables, the argument contract and the meter's arithmetic - no GPU needed.

Every C call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import perturb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
EINVAL = -22
FAKE = 1 << 30          # non-NULL pointer values the argument checks accept (nothing is ever read from them)
SIZES = [1, 2, 63, 64, 65, 197, 1025]


def _lib():
    from mfvit import _lib
    return _lib


def _perturb():
    from mfvit import perturb
    return perturb


# ------------------------------------------------------------------------------------------------------- the rank rule
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("kind", R.RANK_KINDS)
def test_rank_reference_is_the_inverse_of_numpys_stable_argsort(kind, P):
    rel = R.rank_inputs(kind, 3, P, seed=P)
    ref = R.ref_rank(rel)
    assert R.rank_mismatch(ref, R.inverse_argsort_rank(rel)) is None
    assert all(sorted(row.tolist()) == list(range(P)) for row in ref)          # a permutation: the order is total


def test_rank_reference_on_a_hand_made_row():
    nan, inf = float("nan"), float("inf")
    rel = np.array([[0.0, nan, -inf, -0.0, 2.0, inf, nan, 2.0]], dtype=np.float32)
    #               inf=0, the 2.0s by index 1, 2, the zeros by index 3, 4, -inf 5, the NaNs by index 6, 7
    assert R.ref_rank(rel).tolist() == [[3, 6, 5, 4, 1, 0, 7, 2]]


@pytest.mark.parametrize("P", SIZES)
def test_rank_differs_from_torch_argsort_exactly_where_nans_are(P):
    rel = R.rank_inputs("special", 6, P, seed=100 + P)
    rel[0] = np.where(np.isnan(rel[0]), 0.5, rel[0])                           # a row without NaN
    rel[1] = np.float32(1.0)
    if P > 1:
        rel[2, P // 2] = np.nan                                                # a row with a NaN and a number
        rel[2, 0] = 7.0
    ref = R.ref_rank(rel)
    order = torch.argsort(torch.from_numpy(rel), dim=1, descending=True, stable=True).numpy()
    tr = np.empty_like(ref)
    for b in range(rel.shape[0]):
        tr[b, order[b]] = np.arange(P, dtype=np.int32)
    for b in range(rel.shape[0]):
        nan = np.isnan(rel[b])
        differs = not np.array_equal(tr[b], ref[b])
        # torch puts NaN first: the two orders agree unless a NaN has a number to be misplaced against
        assert differs == bool(nan.any() and not nan.all()), (b, rel[b], tr[b], ref[b])


def test_the_gpu_tests_comparison_catches_wrong_rank_variants():
    rel = R.rank_inputs("special", 3, 65, seed=5)
    rel[1] = R.rank_inputs("few_values", 1, 65, seed=6)[0]
    ref = R.ref_rank(rel)
    assert R.rank_mismatch(ref.copy(), ref) is None
    # a tie broken by the higher index
    hi_ties = R.inverse_argsort_rank(rel[:, ::-1])[:, ::-1]                    # stable from the right: ties go to the higher index first
    assert sorted(hi_ties[1].tolist()) == list(range(65)) and R.rank_mismatch(hi_ties, ref) is not None
    # NaN ranked first (torch's order)
    order = torch.argsort(torch.from_numpy(rel), dim=1, descending=True, stable=True).numpy()
    nan_first = np.empty_like(ref)
    for b in range(3):
        nan_first[b, order[b]] = np.arange(65, dtype=np.int32)
    assert R.rank_mismatch(nan_first, ref) is not None
    # a rank off by one in the last patch of the last image
    off = ref.copy()
    off[-1, -1] += 1
    assert R.rank_mismatch(off, ref) is not None
    # ... and the dtype and the shape
    assert R.rank_mismatch(ref.astype(np.int64), ref) is not None and R.rank_mismatch(ref[:, :-1], ref) is not None


# ------------------------------------------------------------------------------------------------------- step_counts / ranges_for
def test_step_counts_truncate_as_the_published_script():
    sc = _perturb().step_counts
    assert sc(196) == [0, 19, 39, 58, 78, 98, 117, 137, 156, 176]
    assert sc(576) == [0, 57, 115, 172, 230, 288, 345, 403, 460, 518]
    assert sc(4) == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3]                             # repeated counts are legal
    assert sc(9) == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert sc(196, (0, .25, .5, 1)) == [0, 49, 98, 196]
    assert sc(196, ks=[0, 1, 1, 196]) == [0, 1, 1, 196]
    assert sc(1) == [0] * 10 and sc(8192, (0, 1.0)) == [0, 8192]


@pytest.mark.parametrize("bad", [dict(fractions=(0.1, 0.2)), dict(fractions=(0, 0.5, 0.4)), dict(fractions=(0, 1.5)), dict(fractions=()),
                                 dict(fractions=(0, float("nan"))), dict(ks=[1, 2]), dict(ks=[0, 3, 2]), dict(ks=[0, 197]), dict(ks=[]),
                                 dict(ks=[0, 1.5]), dict(ks=[0, True]), dict(fractions=(0, 1), ks=[0, 1])])
def test_step_counts_refuse_bad_schedules(bad):
    with pytest.raises(ValueError):
        _perturb().step_counts(196, **bad)


def test_step_counts_refuse_bad_patch_counts():
    for P in (0, -1, 8193, 1.5, None):
        with pytest.raises(ValueError):
            _perturb().step_counts(P)


def test_ranges_for_the_three_modes_at_the_ends():
    rf = _perturb().ranges_for
    P = 196
    r = rf(P, [0, 19, P], "positive")
    assert r.dtype == torch.int32 and r.shape == (3, 2) and not r.is_cuda
    assert r.tolist() == [[0, 0], [0, 19], [0, P]]
    assert rf(P, [0, 19, P], "negative").tolist() == [[P, P], [P - 19, P], [0, P]]
    assert rf(P, [0, 19, P], "insertion").tolist() == [[0, P], [19, P], [P, P]]
    # k = 0 removes nothing in the removal modes and everything in insertion; k = P the other way round
    for mode, k, removed in (("positive", 0, 0), ("negative", 0, 0), ("insertion", 0, P), ("positive", P, P), ("negative", P, P),
                             ("insertion", P, 0)):
        lo, hi = rf(P, [k], mode)[0].tolist()
        assert 0 <= lo <= hi <= P and hi - lo == removed
    for bad in (dict(P=P, ks=[0], mode="deletion"), dict(P=P, ks=[P + 1], mode="positive"), dict(P=P, ks=[-1], mode="negative"),
                dict(P=P, ks=[], mode="positive"), dict(P=0, ks=[0], mode="positive"), dict(P=P, ks=[0.5], mode="positive")):
        with pytest.raises(ValueError):
            rf(**bad)


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_lib_binds_the_entry_points():
    L = _lib()
    h = L.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mfvit.h")).read(), flags=re.S)
    for name, arity in (("mfvit_patch_rank", 6), ("mfvit_patch_perturb", 11), ("mfvit_perturb_score", 10)):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/mfvit.h"
        assert name in L.SIGNATURES and hasattr(h, name)
        assert len(L.SIGNATURES[name][1]) == arity
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(decl.split(",")) == arity
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5                          # additive: the version stays


# (rel, ld, rank, B, P)
RANK_INVALID = {
    "rel_null": (None, 196, FAKE, 2, 196),
    "rank_null": (FAKE, 196, None, 2, 196),
    "B_zero": (FAKE, 196, FAKE, 0, 196),
    "B_negative": (FAKE, 196, FAKE, -1, 196),
    "B_65536": (FAKE, 196, FAKE, 65536, 196),
    "P_zero": (FAKE, 196, FAKE, 2, 0),
    "P_negative": (FAKE, 196, FAKE, 2, -4),
    "P_8193": (FAKE, 8193, FAKE, 2, 8193),
    "ld_below_P": (FAKE, 195, FAKE, 2, 196),
}


@pytest.mark.parametrize("case", sorted(RANK_INVALID))
def test_patch_rank_refuses_invalid_calls_without_a_device(case):
    rel, ld, rank, B, P = RANK_INVALID[case]
    assert _lib().lib().mfvit_patch_rank(rel, ld, rank, B, P, None) == EINVAL


B_, C_, H_, W_, S_ = 2, 3, 32, 48, 4
IMG_BYTES = B_ * C_ * H_ * W_ * 4
IMG, OUT, RANK, STEPS, FILL = FAKE, FAKE + 2 * IMG_BYTES, FAKE + 16 * IMG_BYTES, FAKE + 17 * IMG_BYTES, FAKE + 18 * IMG_BYTES
# (img, rank, steps, fill, out, B, C, H, W, S)
PERTURB_INVALID = {
    "img_null": (None, RANK, STEPS, FILL, OUT, B_, C_, H_, W_, S_),
    "rank_null": (IMG, None, STEPS, FILL, OUT, B_, C_, H_, W_, S_),
    "steps_null": (IMG, RANK, None, FILL, OUT, B_, C_, H_, W_, S_),
    "fill_null": (IMG, RANK, STEPS, None, OUT, B_, C_, H_, W_, S_),
    "out_null": (IMG, RANK, STEPS, FILL, None, B_, C_, H_, W_, S_),
    "H_not_multiple_of_16": (IMG, RANK, STEPS, FILL, OUT, B_, C_, 40, W_, S_),
    "W_not_multiple_of_16": (IMG, RANK, STEPS, FILL, OUT, B_, C_, H_, 56, S_),
    "H_zero": (IMG, RANK, STEPS, FILL, OUT, B_, C_, 0, W_, S_),
    "W_negative": (IMG, RANK, STEPS, FILL, OUT, B_, C_, H_, -16, S_),
    "P_above_8192": (IMG, RANK, STEPS, FILL, FAKE + (1 << 40), 1, 1, 16 * 91, 16 * 91, 1),
    "B_zero": (IMG, RANK, STEPS, FILL, OUT, 0, C_, H_, W_, S_),
    "C_zero": (IMG, RANK, STEPS, FILL, OUT, B_, 0, H_, W_, S_),
    "S_zero": (IMG, RANK, STEPS, FILL, OUT, B_, C_, H_, W_, 0),
    "S_negative": (IMG, RANK, STEPS, FILL, OUT, B_, C_, H_, W_, -1),
    "B_65536": (IMG, RANK, STEPS, FILL, FAKE + (1 << 40), 65536, 1, 16, 16, 1),
    "S_65536": (IMG, RANK, STEPS, FILL, FAKE + (1 << 40), 1, 1, 16, 16, 65536),
    "CHW_above_2_30": (IMG, RANK, STEPS, FILL, FAKE + (1 << 40), 1, 4100, 512, 512, 1),
    "out_is_img": (IMG, RANK, STEPS, FILL, IMG, B_, C_, H_, W_, S_),
    "out_overlaps_img_tail": (IMG, RANK, STEPS, FILL, IMG + IMG_BYTES - 16, B_, C_, H_, W_, S_),
    "img_inside_out": (IMG + 2 * IMG_BYTES, RANK, STEPS, FILL, IMG, B_, C_, H_, W_, S_),
    "out_ends_inside_img": (IMG + S_ * IMG_BYTES - 16, RANK, STEPS, FILL, IMG, B_, C_, H_, W_, S_),
}


@pytest.mark.parametrize("case", sorted(PERTURB_INVALID))
def test_patch_perturb_refuses_invalid_calls_without_a_device(case):
    img, rank, steps, fill, out, B, C, H, W, S = PERTURB_INVALID[case]
    assert _lib().lib().mfvit_patch_perturb(img, rank, steps, fill, out, B, C, H, W, S, None) == EINVAL


# (logits, ld, target, S, B, C, correct, sums, nonfinite)
SCORE_INVALID = {
    "logits_null": (None, 3, FAKE, 4, 7, 3, FAKE, FAKE, FAKE),
    "target_null": (FAKE, 3, None, 4, 7, 3, FAKE, FAKE, FAKE),
    "correct_null": (FAKE, 3, FAKE, 4, 7, 3, None, FAKE, FAKE),
    "sums_null": (FAKE, 3, FAKE, 4, 7, 3, FAKE, None, FAKE),
    "nonfinite_null": (FAKE, 3, FAKE, 4, 7, 3, FAKE, FAKE, None),
    "S_zero": (FAKE, 3, FAKE, 0, 7, 3, FAKE, FAKE, FAKE),
    "B_zero": (FAKE, 3, FAKE, 4, 0, 3, FAKE, FAKE, FAKE),
    "C_zero": (FAKE, 3, FAKE, 4, 7, 0, FAKE, FAKE, FAKE),
    "S_negative": (FAKE, 3, FAKE, -4, 7, 3, FAKE, FAKE, FAKE),
    "ld_below_C": (FAKE, 2, FAKE, 4, 7, 3, FAKE, FAKE, FAKE),
}


@pytest.mark.parametrize("case", sorted(SCORE_INVALID))
def test_perturb_score_refuses_invalid_calls_without_a_device(case):
    logits, ld, target, S, B, C, correct, sums, nonfinite = SCORE_INVALID[case]
    assert _lib().lib().mfvit_perturb_score(logits, ld, target, S, B, C, correct, sums, nonfinite, None) == EINVAL


# ------------------------------------------------------------------------------------------------------- argument errors of the Python layer
def test_wrapper_argument_errors_come_before_any_launch():
    p = _perturb()
    MfvitError = _lib().MfvitError
    for bad in (torch.zeros(4), torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, dtype=torch.int64), torch.zeros(0, 4), torch.zeros(2, 8193), [[1.0]]):
        with pytest.raises(ValueError):
            p.patch_rank(bad)
    with pytest.raises(MfvitError):
        p.patch_rank(torch.zeros(2, 4))                                        # valid arguments, CPU tensor: loud failure, no fallback
    with pytest.raises(MfvitError):
        p.patch_rank(torch.zeros(2, 2, 2, dtype=torch.float64))
    img, rank = torch.zeros(2, 3, 32, 48), torch.zeros(2, 6, dtype=torch.int32)
    good = p.ranges_for(6, [0, 3], "positive")
    for kw in (dict(img=torch.zeros(3, 32, 48)), dict(img=torch.zeros(2, 3, 30, 48)), dict(img=torch.zeros(2, 3, 32, 40)),
               dict(img=torch.zeros(0, 3, 32, 48)), dict(rank=rank.long()), dict(rank=torch.zeros(2, 5, dtype=torch.int32)),
               dict(rank=torch.zeros(3, 6, dtype=torch.int32)), dict(ranges=[[0, 7]]), dict(ranges=[[3, 2]]), dict(ranges=[[-1, 2]]),
               dict(ranges=[0, 3]), dict(ranges=[[0.0, 3.0]]), dict(ranges=torch.zeros(0, 2, dtype=torch.int32)), dict(fill=[0.1, 0.2]),
               dict(fill=torch.zeros(4))):
        args = dict(img=img, rank=rank, ranges=good, fill=None)
        args.update(kw)
        with pytest.raises(ValueError):
            p.perturb_patches(**args)
    for fill in (None, 0.5, [0.1, 0.2, 0.3], torch.ones(3)):
        with pytest.raises(MfvitError):
            p.perturb_patches(img, rank, good, fill)
    z, t = torch.zeros(4, 7, 3), torch.zeros(7, dtype=torch.int64)
    c, s, n = torch.zeros(4, dtype=torch.int64), torch.zeros(4, 2, dtype=torch.float64), torch.zeros(4, dtype=torch.int64)
    for kw in (dict(logits=z[0]), dict(logits=z.double()), dict(target=t.int()), dict(target=t[:6]), dict(correct=c[:3]), dict(correct=c.int()),
               dict(sums=s.float()), dict(sums=s[:, 0]), dict(nonfinite=n[:2]), dict(logits=torch.zeros(4, 0, 3), target=t[:0])):
        args = dict(logits=z, target=t, correct=c, sums=s, nonfinite=n)
        args.update(kw)
        with pytest.raises(ValueError):
            p.perturb_score(**args)
    with pytest.raises(MfvitError):
        p.perturb_score(z, t, c, s, n)


def test_meter_argument_errors():
    p = _perturb()
    for bad in (0, -1, 1.5, None):
        with pytest.raises(ValueError):
            p.PerturbationMeter(bad)
    with pytest.raises(ValueError):
        p.PerturbationMeter(3, fractions=(0, 1))
    m = p.PerturbationMeter(4, fractions=(0, .25, .5, 1))
    with pytest.raises(ValueError):
        m.set_fractions((0, .25, .5, .75))                                     # a meter accumulates ONE curve
    m.set_fractions((0, .25, .5, 1))
    with pytest.raises(ValueError):
        m.compute()                                                            # nothing scored yet
    z, t = torch.zeros(4, 7, 3), torch.zeros(7, dtype=torch.int64)
    for logits, target in ((z[:3], t), (z[0], t), (z, t[:6]), (z, t.int()), (z, t + 3), (z, t - 1)):
        with pytest.raises(ValueError):
            m.update(logits, target)
    with pytest.raises(_lib().MfvitError):
        m.update(z, t)
    assert m.n == 0


class _FakeEncoder:
    """What perturbation_test reads from an encoder before anything is launched."""
    _feat_cache = None

    def _head_width(self):
        return 3

    def modules(self):
        return []


def test_perturbation_test_argument_errors_come_before_any_launch():
    p = _perturb()
    model = _FakeEncoder()
    img, maps = torch.zeros(2, 3, 32, 48), torch.zeros(2, 2, 3)
    for kw in (dict(img=torch.zeros(3, 32, 48)), dict(img=torch.zeros(2, 3, 33, 48)), dict(maps=None), dict(maps=torch.zeros(2, 3, 2)),
               dict(maps=torch.zeros(2, 5)), dict(maps=torch.zeros(3, 6)), dict(maps=torch.zeros(2, 6, dtype=torch.int32)), dict(mode="delete"),
               dict(fractions=(0.5, 1)), dict(ks=[0, 7]), dict(max_batch=1), dict(max_batch=2.5), dict(target=3), dict(target=-1),
               dict(target=1.0), dict(target=torch.tensor([0, 1, 2])), dict(target=torch.tensor([0.0, 1.0])),
               dict(meter=p.PerturbationMeter(3)), dict(meter="meter"), dict(meter=p.PerturbationMeter(10, fractions=[0.0] * 10))):
        args = dict(model=model, img=img, maps=maps)
        args.update(kw)
        with pytest.raises(ValueError):
            p.perturbation_test(**args)
    with pytest.raises(_lib().MfvitError):
        p.perturbation_test(model, img, maps)                                  # valid arguments, CPU tensors
    with pytest.raises(_lib().MfvitError):
        p.perturbation_test(model, img, maps.view(2, 6), target=torch.tensor([0, 2]), mode="insertion", ks=[0, 6], max_batch=5)


def test_two_stream_perturbation_test_argument_errors():
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    backs = [vits.vit_small(num_classes=3, depth=1) for _ in range(3)]
    model = fus.Fus_CrossViT(backs[0], backs[1])
    img, m = torch.zeros(2, 3, 224, 224), torch.zeros(2, 14, 14)
    with pytest.raises(ValueError, match="not the encoder"):
        model.perturbation_test(backs[0], backs[2], img, img, (m, m))
    with pytest.raises(ValueError, match="same number"):
        model.perturbation_test(backs[0], backs[1], img, img[:1], (m, m))
    for kw in (dict(maps=(None, None)), dict(maps=m), dict(maps=(m,)), dict(maps=(m, m[:, :13])), dict(maps=(m[:1], None)), dict(fill=0.5),
               dict(fill=(0.0, 0.0, 0.0)), dict(mode="both"), dict(target=3), dict(max_batch=1), dict(fractions=(0.2,))):
        args = dict(maps=(m, None))
        args.update(kw)
        with pytest.raises(ValueError):
            model.perturbation_test(backs[0], backs[1], img, img, **args)
    with pytest.raises(_lib().MfvitError):
        model.perturbation_test(backs[0], backs[1], img, img, (m, None))       # valid arguments, CPU tensors
    assert all(b.training for b in backs) and model.training


# ------------------------------------------------------------------------------------------------------- the meter's arithmetic
def test_auc_is_the_trapezoid_over_the_fractions_divided_by_their_span():
    p = _perturb()
    trapz = getattr(np, "trapezoid", None) or np.trapz
    x = [0.0, 0.1, 0.25, 0.5, 0.5, 0.9]                                         # uneven, one repeated fraction
    acc = [1.0, 0.9, 0.9, 0.4, 0.3, 0.0]
    prob = [0.93, 0.71, 0.65, 0.33, 0.2, 0.05]
    n = 10
    res = p.PerturbationMeter.result_from([round(a * n) for a in acc], [0] * 6, [[q * n, 2.0 * n] for q in prob], n, x)
    assert res.auc_accuracy == pytest.approx(trapz(acc, x) / 0.9, rel=1e-14)
    assert res.auc_prob == pytest.approx(trapz(prob, x) / 0.9, rel=1e-14)
    # a constant curve has AUC = its value, whatever the span
    flat = p.PerturbationMeter.result_from([5, 5, 5], [0, 0, 0], [[2.5, 0.0]] * 3, 10, [0.0, 0.3, 0.6])
    assert flat.auc_accuracy == pytest.approx(0.5, rel=1e-15) and flat.auc_prob == pytest.approx(0.25, rel=1e-15)
    # an empty span has no area; no fractions, no AUC
    assert np.isnan(p.PerturbationMeter.result_from([5, 5], [0, 0], [[1.0, 0.0]] * 2, 10, [0.0, 0.0]).auc_prob)
    assert p.PerturbationMeter.result_from([5], [0], [[1.0, 0.0]], 10).auc_accuracy is None


def test_meter_compute_on_hand_built_accumulators():
    p = _perturb()
    S, n = 3, 8
    m = p.PerturbationMeter(S, fractions=(0, .5, 1))
    sums = torch.tensor([[6.5, 12.0], [3.25, -4.0], [0.125, -20.0]], dtype=torch.float64)
    m._buf = torch.cat([torch.tensor([7, 4, 1]), torch.tensor([0, 1, 2]), sums.view(-1).view(torch.int64)])     # correct | nonfinite | sums
    m.n = n
    c, nf, s = m._views()
    assert c.tolist() == [7, 4, 1] and nf.tolist() == [0, 1, 2] and torch.equal(s, sums)
    res = m.compute()
    assert res.n == n and res.fractions == [0.0, 0.5, 1.0] and res.nonfinite == [0, 1, 2]
    assert res.accuracy == [7 / 8, 4 / 8, 1 / 8]
    assert res.mean_prob == [6.5 / 8, 3.25 / 8, 0.125 / 8]
    assert res.mean_logit == [12.0 / 8, -4.0 / 8, -20.0 / 8]
    assert res.auc_accuracy == pytest.approx((7 / 8 + 2 * 4 / 8 + 1 / 8) / 4, rel=1e-15)
    assert res.auc_prob == pytest.approx((6.5 + 2 * 3.25 + 0.125) / 8 / 4, rel=1e-15)
    assert set(res.as_dict()) >= {"accuracy", "mean_prob", "mean_logit", "fractions", "n", "nonfinite", "auc_accuracy", "auc_prob"}
    m.reset()
    assert m.n == 0 and m._buf is None and m.fractions == [0.0, 0.5, 1.0]


def test_reference_score_on_a_hand_made_case():
    z = np.array([[[0.0, 0.0], [1.0, 3.0], [np.inf, 0.0]]], dtype=np.float32)                                    # a tie, a clear row, a non-finite row
    correct, nonfinite, sums = R.ref_score(z, [0, 0, 1])
    assert correct == [1] and nonfinite == [1]                                                                  # the tie goes to class 0
    assert sums[0][0] == pytest.approx(0.5 + 1.0 / (1.0 + np.exp(2.0)), rel=1e-15) and sums[0][1] == 1.0
