"""ROC / PR curves, operating points and calibration (include/mfvit.h: mfvit_curve_counts, mfvit_boot_points, mfvit_calib_sums;
mfvit.evalstats): the brute-force restatement of tests/opcurve_ref.py pinned to the installed scikit-learn and to torch.softmax, the host
arithmetic on fabricated counts, the gate's power against wrong variants, and the argument contract of the C ABI - no GPU needed.

Every C call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import ctypes
import math

import numpy as np
import pytest

import evalstats_ref as E
import opcurve_ref as O

EINVAL = -22
FAKE = 1 << 30
U = 2.0 ** -53                    # the unit roundoff of float64


def _es():
    from mfvit import evalstats
    return evalstats


def _lib():
    from mfvit import _lib
    return _lib.lib()


def _cases():
    for n, C, M, kind, lkind in ((1, 1, 1, "gauss", "random"), (2, 2, 1, "ties", "random"), (61, 3, 2, "ties", "random"), (200, 4, 1, "gauss", "outside"),
                                 (300, 3, 1, "equal", "random"), (257, 2, 2, "ties", "missing")):
        yield (n, C, M, kind, lkind) + E.case(n, C, M, kind, lkind, 11 * n + C)


# ------------------------------------------------------------------------------------------------------- the restatement against scikit-learn
def test_curve_counts_are_sklearns_binary_clf_curve_and_the_host_curves_are_sklearns():
    from sklearn import metrics as skm
    es = _es()
    seen = 0
    for n, C, M, kind, lkind, s, t in _cases():
        thr, tp, fp, nthr, nnan, npos = O.curve_counts(s, t)
        u2, _ = E.u2_brute(s, t, np.ones(n, dtype=np.int64))
        assert (nnan == 0).all() and (npos == [(t == c).sum() for c in range(C)]).all()
        for m in range(M):
            for c in range(C):
                y, G = (t == c).astype(np.int64), int(nthr[m, c])
                th, a, b = thr[m, c, :G], tp[m, c, :G].astype(np.float64), fp[m, c, :G].astype(np.float64)
                assert np.isnan(thr[m, c, G:]).all() and not tp[m, c, G:].any() and not fp[m, c, G:].any()
                P, N = int(npos[c]), n - int(npos[c])
                if not P or not N:
                    continue                                             # scikit-learn warns and returns NaN rates; the AUC is undefined
                seen += 1
                for drop in (True, False):
                    fpr, tpr, thresholds = skm.roc_curve(y, s[m, :, c], drop_intermediate=drop)
                    got = es.roc_from_counts(th, a, b, drop)
                    np.testing.assert_array_equal(got.thresholds.view(np.int32), np.asarray(thresholds, dtype=np.float32).view(np.int32))
                    np.testing.assert_array_equal(got.fpr, fpr)          # exactly equal in float64
                    np.testing.assert_array_equal(got.tpr, tpr)
                    assert got.fpr.dtype == np.float64
                # the area under the curve is the pair count
                full = es.roc_from_counts(th, a, b, False)
                assert abs(skm.auc(full.fpr, full.tpr) - int(u2[m, c]) / (2.0 * P * N)) <= 4 * (G + 2) * U
                for drop in (False, True):
                    prec, rec, thresholds = skm.precision_recall_curve(y, s[m, :, c], drop_intermediate=drop)
                    got = es.pr_from_counts(th, a, b, drop)
                    np.testing.assert_array_equal(got.precision, prec)
                    np.testing.assert_array_equal(got.recall, rec)
                    np.testing.assert_array_equal(got.thresholds.view(np.int32), np.asarray(thresholds, dtype=np.float32).view(np.int32))
                # average precision.  scikit-learn rounds every recall tp_k / P (relative error U each), so each of its G differences carries an
                # absolute error of up to 2 U and its sum up to 2 G U; ours has one division and one product per term and a pairwise sum:
                # (3 + log2 G) U relative to a value <= 1.  Bound: (2 G + log2 G + 4) U.
                ap = es.ap_from_counts(a, b)
                assert abs(ap - skm.average_precision_score(y, s[m, :, c])) <= (2 * G + math.log2(G + 1) + 4) * U
    assert seen >= 10


def test_zero_signs_and_the_first_holder_rule():
    s = np.array([0.5, -0.0, 0.0, np.nan, -0.0, 0.5, -1.0], dtype=np.float32).reshape(1, 7, 1)
    t = np.array([0, 0, 1, 0, 5, -1, 0], dtype=np.int64)
    thr, tp, fp, nthr, nnan, npos = O.curve_counts(s, t)
    assert nthr[0, 0] == 3 and nnan[0, 0] == 1 and npos[0] == 4
    assert thr[0, 0, :3].tolist() == [0.5, 0.0, -1.0] and np.signbit(thr[0, 0, 1])         # -0.0 comes first in index order
    assert tp[0, 0, :3].tolist() == [1, 2, 3] and fp[0, 0, :3].tolist() == [1, 3, 3]       # the NaN-scored positive is above no threshold
    with pytest.raises(ValueError):
        _es()._column(_es().CurveCounts(thr, tp, fp, nthr, nnan, npos, 7), 0, 0)


# ------------------------------------------------------------------------------------------------------- operating points
def test_weighted_points_by_hand():
    # scores 4 3 3 2 1 (labels + - + - +), unit weights: candidates inf 4 3 2 1 -> TP 0 1 2 2 3, FP 0 0 1 2 2
    s = np.array([4, 3, 3, 2, 1], dtype=np.float32).reshape(1, 5, 1)
    t = np.array([0, 1, 0, 1, 0], dtype=np.int64)
    at = [("specificity", 1.0), ("specificity", 0.5), ("specificity", 0.0), ("sensitivity", 0.0), ("sensitivity", 0.5), ("sensitivity", 1.0),
          ("threshold", 3.0), ("threshold", 9.0), ("threshold", -9.0), ("threshold", float("nan"))]
    req = _es().encode_requests(at)
    np.testing.assert_array_equal(req, O.request_rows(at))
    assert req[:6].tolist() == [[0, 0, 1], [0, 1, 2], [0, 1, 1], [1, 0, 1], [1, 1, 2], [1, 1, 1]]
    tp, fp, thr, npos = O.boot_points(s, t, seed=1, r0=0, R=1, stratified=False, requests=req)
    assert npos.tolist() == [[3]]
    assert tp[0, 0, 0].tolist() == [1, 2, 3, 0, 2, 3, 2, 0, 3, 0]
    assert fp[0, 0, 0].tolist() == [0, 1, 2, 0, 1, 2, 1, 0, 2, 0]
    assert thr[0, 0, 0].tolist() == [4, 3, 1, np.inf, 3, 1, 3, np.inf, 1, np.inf]


def test_replicate_zero_with_a_threshold_request_is_the_curve():
    for n, C, M, kind, lkind in ((40, 2, 2, "special", "outside"), (90, 3, 1, "ties", "missing")):
        s, t = E.case(n, C, M, kind, lkind, n)
        thr, tp, fp, nthr, _, npos = O.curve_counts(s, t)
        for m in range(M):
            for c in range(C):
                G = int(nthr[m, c])
                req = np.array([(2, int(thr[m, c, k:k + 1].view(np.int32)[0]), 0) for k in range(G)], dtype=np.int32)
                btp, bfp, bthr, bnpos = O.boot_points(s[m:m + 1, :, c:c + 1], (t == c).astype(np.int64) - 1, 0, 0, 1, False, req)
                np.testing.assert_array_equal(btp[0, 0, 0], tp[m, c, :G])
                np.testing.assert_array_equal(bfp[0, 0, 0], fp[m, c, :G])
                np.testing.assert_array_equal(bthr[0, 0, 0].view(np.int32), thr[m, c, :G].view(np.int32))


def test_point_statistics_intervals_and_pairs_on_fabricated_counts():
    es = _es()
    n, R = 20, 5
    npos = np.array([[8], [8], [0], [20], [10]], dtype=np.int64)                             # a replicate without positives, one without negatives
    tp = np.array([4, 8, 0, 10, 5], dtype=np.int64).reshape(R, 1, 1, 1)
    fp = np.array([3, 0, 5, 0, 0], dtype=np.int64).reshape(R, 1, 1, 1)
    st = es.point_stats(tp, fp, npos, n)
    np.testing.assert_array_equal(st["sensitivity"].ravel(), [0.5, 1.0, np.nan, 0.5, 0.5])
    np.testing.assert_array_equal(st["specificity"].ravel(), [0.75, 1.0, 0.75, np.nan, 1.0])
    np.testing.assert_array_equal(st["ppv"].ravel(), [4 / 7, 1.0, 0.0, 1.0, 1.0])
    np.testing.assert_array_equal(st["npv"].ravel(), [9 / 13, 1.0, 1.0, 0.0, 10 / 15])
    tp2 = np.concatenate([tp, tp // 2], axis=1)
    fp2 = np.concatenate([fp, fp], axis=1)
    thr = np.zeros((R, 2, 1, 1), dtype=np.float32)
    thr[0, :, 0, 0] = (0.25, 0.75)
    op = es.summarize_points(tp2, fp2, thr, npos, n, [("threshold", 0.25)], level=0.5, names=["a", "b"])
    sa = op.models["a"]["sensitivity"]
    assert sa.point.shape == (1, 1) and sa.point[0, 0] == 0.5 and sa.dropped[0, 0] == 1
    lo, hi, dropped = E.interval([1.0, np.nan, 0.5, 0.5], 0.5)
    assert (sa.lo[0, 0], sa.hi[0, 0]) == (lo, hi) and op.models["b"]["threshold"][0, 0] == 0.75 and op.n_boot == R - 1
    d = op.pairs[("a", "b")]["sensitivity"]
    p, used = E.p_two_sided([0.5, np.nan, 0.25, 0.25])
    assert d.point[0, 0] == 0.25 and d.p[0, 0] == p and d.used[0, 0] == used == 3
    assert op.pairs[("a", "b")]["specificity"].point[0, 0] == 0.0 and set(op.pairs) == {("a", "b"), ("b", "a")}


# ------------------------------------------------------------------------------------------------------- calibration
def test_calibration_restatement_against_torch_softmax():
    es = _es()
    rng = np.random.Generator(np.random.PCG64(5))
    for n, C, T, NB in ((500, 3, 1.0, 15), (300, 5, 2.5, 10), (64, 2, 0.5, 1)):
        z = (3.0 * rng.standard_normal((n, C))).astype(np.float32)
        y = rng.integers(0, C, n)
        ref = O.calib_sums(z, y, [T], NB)
        assert O.edge_margin(ref["conf"][0, 0], NB) > 1e-9 or NB == 1
        cal = es.calibration_from_sums(ref["bin_n"][0, 0], ref["bin_hit"][0, 0], ref["bin_conf"][0, 0], ref["sums"][0, 0], ref["skipped"][0], n, T)
        ece, mce, brier, nll = O.calibration_direct(z, y, T, NB)
        # n terms each within a few U of the direct form, sums of values <= 1 (log terms: <= ~50): 64 n U covers them
        tol = 64 * n * U
        assert abs(cal.ece - ece) < tol and abs(cal.mce - mce) < tol and abs(cal.brier - brier) < tol and abs(cal.nll - nll) < 50 * tol
        assert cal.used == n and cal.skipped == 0 and int(cal.bin_count.sum()) == n
    z[3, 1], z[7, 0], y[11] = np.inf, np.nan, C
    ref = O.calib_sums(z, y, [0.5, 1.0], 4)
    assert ref["skipped"].tolist() == [3] and ref["bin_n"].sum(2).tolist() == [[n - 3, n - 3]]
    # a saturated row lands in the last bin with confidence exactly 1; one class: confidence 1, NLL 0
    one = O.calib_sums(np.array([[200.0, -200.0, 0.0]], dtype=np.float32), np.array([0]), [1.0], 15)
    assert one["conf"][0, 0, 0] == 1.0 and one["bin_n"][0, 0, 14] == 1 and one["sums"][0, 0, 0] == 0.0
    c1 = O.calib_sums(np.zeros((5, 1), dtype=np.float32), np.zeros(5, dtype=np.int64), [3.0], 7)
    assert c1["bin_n"][0, 0].tolist() == [0] * 6 + [5] and c1["sums"][0, 0].tolist() == [0.0, 0.0, 0.0]


def test_fit_temperature_brackets_the_minimiser_scipy_finds():
    from scipy.optimize import minimize_scalar
    es = _es()
    rng = np.random.Generator(np.random.PCG64(9))
    n, C = 400, 3
    y = rng.integers(0, C, n)
    base = rng.standard_normal((n, C))
    base[np.arange(n), y] += 1.5
    for factor in (0.4, 1.0, 3.0):
        z = (factor * base).astype(np.float32)
        launches = []

        def slope_at(t):
            launches.append(len(t))
            return O.calib_sums(z, y, t, 1)["sums"][0, :, 2]
        lo, hi = es.refine_bracket(slope_at, 0.05, 20.0)
        assert 0 < hi - lo <= 1e-6 * lo and max(launches) <= 16 and len(launches) <= 8
        nll = lambda T: O.calib_sums(z, y, [np.float32(T)], 1)["sums"][0, 0, 0]
        got = minimize_scalar(lambda b: _nll64(z, y, b), bounds=(1 / 20.0, 1 / 0.05), method="bounded", options={"xatol": 1e-10})
        # the minimiser lies inside the bracket up to scipy's own tolerance: near the minimum the NLL is flat to second order, so a bounded search
        # on VALUES resolves beta to about sqrt(U) relative (1.5e-8), not to xatol; tolerance = the bracket width + 1e-7 relative for that
        T_ref = 1.0 / got.x
        assert lo - 1e-7 * lo - (hi - lo) <= T_ref <= hi + 1e-7 * hi + (hi - lo), (lo, hi, T_ref)
        assert nll(0.5 * (lo + hi)) <= min(nll(lo * 0.99), nll(hi * 1.01))
    # the sign never changes: the bracket's end
    assert es.refine_bracket(lambda t: -np.ones(len(t)), 0.05, 20.0) == (float(np.float32(0.05)), float(np.float32(0.05)))
    assert es.refine_bracket(lambda t: np.ones(len(t)), 0.05, 20.0) == (20.0, 20.0)
    assert es.refine_bracket(lambda t: 1.0 - np.asarray(t, dtype=np.float64), 0.5, 16.0) == (1.0, 1.0)        # a candidate with slope 0


def _nll64(z, y, beta):
    d = z.astype(np.float64) * beta
    d = d - d.max(1, keepdims=True)
    return float((np.log(np.exp(d).sum(1)) - d[np.arange(len(y)), y]).sum())


# ------------------------------------------------------------------------------------------------------- the gate's power
def test_wrong_variants_fail_the_gate():
    s, t = E.case(120, 3, 2, "special", "outside", 77)
    good = O.curve_counts(s, t)
    for variant in ("gt", "nan_pred"):
        bad = O.curve_counts(s, t, variant)
        assert any((g != b).any() for g, b in zip(good[1:3], bad[1:3])), variant
    at = [("specificity", 0.9), ("sensitivity", 0.9), ("sensitivity", 1 / 3), ("threshold", 0.25)]
    req = O.request_rows(at)
    good = O.boot_points(s, t, 5, 0, 4, False, req)
    for variant in ("gt", "floor", "nan_pred"):
        bad = O.boot_points(s, t, 5, 0, 4, False, req, variant)
        assert (good[0] != bad[0]).any() or (good[1] != bad[1]).any(), variant
    # [lo, hi) bins: a confidence exactly on an edge moves (probabilities 0.5 / 0.5 with two bins, and the saturated row)
    z = np.array([[1.0, 1.0], [300.0, -300.0], [0.3, -0.2]], dtype=np.float32)
    y = np.array([0, 0, 1], dtype=np.int64)
    a, b = O.calib_sums(z, y, [1.0], 2), O.calib_sums(z, y, [1.0], 2, "lo_hi_open")
    assert a["bin_n"][0, 0].tolist() == [1, 2] and (a["bin_n"] != b["bin_n"]).any()


# ------------------------------------------------------------------------------------------------------- requests and the C ABI's refusals
def test_encode_requests():
    es = _es()
    req = es.encode_requests([("specificity", 0.95), ("sensitivity", 0.9), ("threshold", -0.0), ("specificity", 1 / 3)])
    assert req.dtype == np.int32 and req[0].tolist() == [0, 1, 20] and req[1].tolist() == [1, 9, 10]
    assert req[2].tolist() == [2, -2 ** 31, 0] and req[3, 2] <= 2 ** 20
    for bad in ([], [("specificity", 1.5)], [("auc", 0.5)], [("threshold", 0.0)] * 65):
        with pytest.raises(Exception):
            es.encode_requests(bad)


def test_argument_errors_are_refused_before_any_gpu_call():
    L = _lib()
    n, C, M, R, Q = 100, 3, 2, 4, 2
    wb = L.mfvit_boot_work_bytes(n, C, M, R)
    assert L.mfvit_abi_version() == 5 and wb > 0

    def curve(**kw):
        a = dict(scores=FAKE, ld=C, ms=n * C, labels=FAKE, n=n, C=C, M=M, work=FAKE, wb=wb, thr=FAKE, tp=FAKE, fp=FAKE, nthr=FAKE, nnan=FAKE, npos=FAKE)
        a.update(kw)
        return L.mfvit_curve_counts(a["scores"], a["ld"], a["ms"], a["labels"], a["n"], a["C"], a["M"], a["work"], a["wb"], a["thr"], a["tp"], a["fp"],
                                    a["nthr"], a["nnan"], a["npos"], None)

    def points(**kw):
        a = dict(scores=FAKE, ld=C, ms=n * C, labels=FAKE, n=n, C=C, M=M, seed=1, r0=0, R=R, strat=0, req=FAKE, Q=Q, work=FAKE, wb=wb, tp=FAKE, fp=FAKE,
                 thr=FAKE, npos=FAKE)
        a.update(kw)
        return L.mfvit_boot_points(a["scores"], a["ld"], a["ms"], a["labels"], a["n"], a["C"], a["M"], a["seed"], a["r0"], a["R"], a["strat"], a["req"],
                                   a["Q"], a["work"], a["wb"], a["tp"], a["fp"], a["thr"], a["npos"], None)

    temps = (ctypes.c_float * 16)(*([1.0] * 16))

    def calib(**kw):
        a = dict(logits=FAKE, ld=C, ms=n * C, labels=FAKE, n=n, C=C, M=M, temps=ctypes.cast(temps, ctypes.c_void_p), Kt=2, NB=15, bin_n=FAKE,
                 bin_hit=FAKE, bin_conf=FAKE, sums=FAKE, skipped=FAKE)
        a.update(kw)
        return L.mfvit_calib_sums(a["logits"], a["ld"], a["ms"], a["labels"], a["n"], a["C"], a["M"], a["temps"], a["Kt"], a["NB"], a["bin_n"],
                                  a["bin_hit"], a["bin_conf"], a["sums"], a["skipped"], None)

    shape = (dict(n=0), dict(n=32769), dict(C=0), dict(C=65), dict(M=0), dict(M=9), dict(ld=C - 1), dict(ms=(n - 1) * C + C - 1), dict(labels=None))
    for kw in shape + (dict(scores=None), dict(work=None), dict(work=FAKE + 8), dict(wb=wb - 1), dict(thr=None), dict(tp=None), dict(fp=None),
                       dict(nthr=None), dict(nnan=None), dict(npos=None)):
        assert curve(**kw) == EINVAL, kw
    for kw in shape + (dict(scores=None), dict(work=None), dict(wb=wb - 1), dict(R=0), dict(r0=-1), dict(r0=2 ** 31 - 1), dict(strat=2), dict(req=None),
                       dict(Q=0), dict(Q=65), dict(tp=None), dict(fp=None), dict(thr=None), dict(npos=None)):
        assert points(**kw) == EINVAL, kw
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        t = (ctypes.c_float * 16)(*([1.0, bad] + [1.0] * 14))
        assert calib(temps=ctypes.cast(t, ctypes.c_void_p)) == EINVAL, bad
    for kw in shape + (dict(logits=None), dict(temps=None), dict(Kt=0), dict(Kt=17), dict(NB=0), dict(NB=65), dict(bin_n=None), dict(bin_hit=None),
                       dict(bin_conf=None), dict(sums=None), dict(skipped=None)):
        assert calib(**kw) == EINVAL, kw
