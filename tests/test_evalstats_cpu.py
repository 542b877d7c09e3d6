"""Bootstrap confidence intervals and DeLong tests (include/mfvit.h: mfvit_boot_counts, mfvit_delong_counts; mfvit.evalstats): the reference
restatement against itself, scikit-learn and the oracle, the gate's power against wrong variants, the argument contract of the C ABI and the
host arithmetic - no GPU needed.

Every C call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import math
import os
import re

import numpy as np
import pytest

import evalstats_ref as E
from oracle import ref_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FAKE = 1 << 30          # a non-NULL, 16-byte aligned pointer value the argument checks accept (nothing is ever read from it)
KINDS = ("gauss", "ties", "equal", "special")
LKINDS = ("random", "outside", "missing")


def _lib():
    from mfvit import _lib
    return _lib


def _es():
    from mfvit import evalstats
    return evalstats


# ------------------------------------------------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("lkind", LKINDS)
@pytest.mark.parametrize("kind", KINDS)
def test_brute_force_and_sort_based_restatements_agree_exactly(kind, lkind):
    for n, C, M in ((1, 1, 1), (2, 2, 1), (61, 3, 2), (200, 4, 1)):
        s, t = E.case(n, C, M, kind, lkind, 7 * n + C)
        for strat in (False, True):
            a = E.boot_counts(s, t, seed=3, r0=0, R=3, stratified=strat, brute=True)
            b = E.boot_counts(s, t, seed=3, r0=0, R=3, stratified=strat, brute=False)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
        for x, y in zip(E.delong_counts(s, t, brute=True), E.delong_counts(s, t, brute=False)):
            np.testing.assert_array_equal(x, y)


def test_hash_matches_a_plain_python_statement():
    def lb(x):
        x ^= x >> 16; x = x * 0x7FEB352D & E.M32; x ^= x >> 15; x = x * 0x846CA68B & E.M32; x ^= x >> 16
        return x
    for x in (0, 1, 0x9E3779B9, 0xFFFFFFFF, 123456789):
        assert int(E.lowbias32(x)) == lb(x)
    seed = 0x0123456789ABCDEF
    assert E.replicate_key(seed, 5) == lb((seed & E.M32) ^ lb(((seed >> 32) + 0x9E3779B9 * 6) & E.M32))
    n, key = 1000, E.replicate_key(seed, 5)
    w = np.zeros(n, dtype=np.int64)
    for k in range(n):
        w[(lb(k ^ key) * n) >> 32] += 1
    np.testing.assert_array_equal(w, E.weights(n, seed, 5))


def test_weights_sum_to_n_and_stratified_weights_keep_every_stratum():
    for n, C, lkind in ((1, 1, "random"), (97, 3, "outside"), (600, 5, "missing")):
        _, t = E.case(n, C, 1, "gauss", lkind, n)
        s = E.strata_of(t, C)
        assert (E.weights(n, 9, 0) == 1).all()
        for r in range(1, 6):
            assert E.weights(n, 9, r).sum() == n
            w = E.weights(n, 9, r, t, C, stratified=True)
            for k in range(C + 1):
                assert w[s == k].sum() == (s == k).sum()
        assert not np.array_equal(E.weights(n, 9, 1), E.weights(n, 9, 2)) or n == 1
        assert not np.array_equal(E.weights(n, 9, 1), E.weights(n, 10, 1)) or n == 1


def test_chunked_calls_concatenate_to_one_call():
    s, t = E.case(83, 3, 2, "ties", "outside", 1)
    for strat in (False, True):
        whole = E.boot_counts(s, t, seed=77, r0=0, R=7, stratified=strat)
        parts = [E.boot_counts(s, t, seed=77, r0=r0, R=R, stratified=strat) for r0, R in ((0, 1), (1, 4), (5, 2))]
        for k in range(3):
            np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts]))


# ------------------------------------------------------------------------------------------------------- against scikit-learn and the oracle
def test_weighted_auc_and_confusion_equal_scikit_learn():
    from sklearn.metrics import confusion_matrix, roc_auc_score
    n, C = 600, 3
    s, t = E.case(n, C, 1, "ties", "random", 42)
    worst = 0.0
    for r in (1, 2, 3):
        w = E.weights(n, 5, r)
        u2, npos = E.u2_brute(s, t, w)
        for c in range(C):
            want = roc_auc_score((t == c).astype(int), s[0, :, c].astype(np.float64), sample_weight=w)
            got = int(u2[0, c]) / (2.0 * int(npos[c]) * (n - int(npos[c])))
            worst = max(worst, abs(got - want))
        want = confusion_matrix(t, E.preds_of(s)[0], labels=list(range(C)), sample_weight=w)
        np.testing.assert_array_equal(E.conf_weighted(s, t, w)[0], want.astype(np.int64))
    assert worst < 1e-12, worst


@pytest.mark.parametrize("kind,lkind", [("gauss", "random"), ("ties", "outside"), ("inf", "missing"), ("zeros", "single")])
def test_replicate_zero_is_the_oracles_epoch_counts(kind, lkind):
    n, C = 300, 3
    s = ref_metrics.edge_scores(n, C, kind, 4)
    t = ref_metrics.edge_labels(n, C, lkind, 4)
    conf, u2, npos = E.boot_counts(s, t, seed=1, r0=0, R=1)
    pairs = ref_metrics.auc_pair_counts(s, t, C)
    assert u2[0, 0].tolist() == [p[0] for p in pairs] and npos[0].tolist() == [p[1] for p in pairs]
    np.testing.assert_array_equal(conf[0, 0], ref_metrics.confusion_matrix(ref_metrics.argmax_first(s), t, C))
    _, _, _, du2, dnpos = E.delong_counts(s, t)
    assert du2[0].tolist() == [p[0] for p in pairs] and dnpos.tolist() == [p[1] for p in pairs]


def test_delong_from_integer_moments_equals_the_psi_matrix_definition():
    n, C, M = 400, 3, 3
    s, t = E.case(n, C, M, "ties", "random", 8)
    _, pos_xy, neg_xy, u2, npos = E.delong_counts(s, t)
    got = E.delong_from_counts(pos_xy, neg_xy, u2, npos, n)
    mine = _es().delong_from_counts(pos_xy, neg_xy, u2, npos, n)
    for c in range(C):
        theta, cov = E.delong_direct(s, t, c)
        np.testing.assert_allclose(got["auc"][:, c], theta, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["cov"][c], cov, rtol=0, atol=1e-14)                 # covariances ~ 1e-4: 1e-14 is 1e-10 relative
    for k, v in (("auc", mine.auc), ("var", mine.var), ("lo", mine.lo), ("hi", mine.hi), ("cov", mine.cov), ("z", mine.z), ("p", mine.p)):
        np.testing.assert_allclose(v, got[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=k)
    assert np.isnan(mine.z[0, 1, 1]) and np.isfinite(mine.z[0, 0, 1]) and mine.z[0, 0, 1] == -mine.z[0, 1, 0]
    # fewer than two positives or negatives: NaN variance
    t2 = np.zeros(5, dtype=np.int64)
    t2[0] = 1
    s2, _ = E.case(5, 2, 1, "gauss", "random", 1)
    _, a, b, c_, d = E.delong_counts(s2, t2)
    r = _es().delong_from_counts(a, b, c_, d, 5)
    assert np.isnan(r.var).all() and np.isfinite(r.auc).all()


# ------------------------------------------------------------------------------------------------------- the gate has teeth
def test_the_bit_exact_gate_catches_wrong_variants():
    n, C = 150, 3
    s, t = E.case(n, C, 1, "special", "outside", 12)
    w = E.weights(n, 3, 1)
    good, _ = E.u2_brute(s, t, w)
    for variant in ("no_tie_credit", "one_sided", "nan_smallest"):
        bad, _ = E.u2_brute(s, t, w, variant=variant)
        assert not np.array_equal(good, bad), variant
    right = E.boot_counts(s, t, seed=3, r0=0, R=4)
    stale = E.boot_counts(s, t, seed=3, r0=0, R=4, key_of=lambda seed, r: E.replicate_key(seed, max(r - 1, 1)))    # replicate r reuses r - 1's key
    assert np.array_equal(right[1][:2], stale[1][:2]) and not np.array_equal(right[1][2:], stale[1][2:])


# ------------------------------------------------------------------------------------------------------- one statistical anchor
def test_bootstrap_standard_deviation_matches_the_delong_standard_error():
    """n = 600, priors .6 / .3 / .1, the true class shifted by +1, class 0, 2,000 replicates: bootstrap sd / DeLong se must lie in [0.85, 1.15].
    The band is a condition, not a measurement; measured for this seeded case: 0.9820."""
    n, C, R = 600, 3, 2000
    rng = np.random.Generator(np.random.PCG64(2024))
    t = rng.choice(C, size=n, p=[0.6, 0.3, 0.1]).astype(np.int64)
    s = rng.standard_normal((1, n, C)).astype(np.float32)
    s[0, np.arange(n), t] += 1.0
    _, pos_xy, neg_xy, u2, npos = E.delong_counts(s, t, brute=False)
    se = math.sqrt(E.delong_from_counts(pos_xy, neg_xy, u2, npos, n)["var"][0, 0])
    aucs = []
    for r in range(1, R + 1):
        w = E.weights(n, 1, r)
        bu2, bnpos = E.u2_sorted(s[:, :, :1], np.where(t == 0, 0, 1), w)
        aucs.append(int(bu2[0, 0]) / (2.0 * int(bnpos[0]) * (n - int(bnpos[0]))))
    ratio = float(np.std(aucs, ddof=1)) / se
    print(f"bootstrap sd / DeLong se = {ratio:.4f}")
    assert 0.85 <= ratio <= 1.15, ratio


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_lib_binds_the_entry_points():
    L = _lib()
    h = L.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mfvit.h")).read(), flags=re.S)
    for name, arity in (("mfvit_boot_work_bytes", 4), ("mfvit_boot_counts", 17), ("mfvit_delong_counts", 15)):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/mfvit.h"
        assert name in L.SIGNATURES and hasattr(h, name)
        assert len(L.SIGNATURES[name][1]) == arity
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(decl.split(",")) == arity
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5                          # additive: the version stays


def test_work_bytes_grow_with_the_replicates_and_refuse_invalid_shapes():
    h = _lib().lib()
    assert h.mfvit_boot_work_bytes(4096, 3, 3, 1) > 0
    assert h.mfvit_boot_work_bytes(4096, 3, 3, 2000) >= h.mfvit_boot_work_bytes(4096, 3, 3, 1)
    assert h.mfvit_boot_work_bytes(4096, 3, 3, 20000) - h.mfvit_boot_work_bytes(4096, 3, 3, 10000) == 10000 * 4096 * 2      # u16 weights
    assert h.mfvit_boot_work_bytes(32768, 64, 8, 1) > 0 and h.mfvit_boot_work_bytes(1, 1, 1, 1) > 0
    for bad in ((0, 3, 3, 1), (32769, 3, 3, 1), (10, 0, 3, 1), (10, 65, 3, 1), (10, 3, 0, 1), (10, 3, 9, 1), (10, 3, 3, 0), (10, 3, 3, -1)):
        assert h.mfvit_boot_work_bytes(*bad) == 0, bad


BIG = 1 << 40       # a work_bytes no layout exceeds
# (scores, ld, model_stride, labels, n, C, M, seed, r0, R, stratified, work, work_bytes, conf, u2, npos)
BOOT_OK = dict(scores=FAKE, ld=3, ms=300, labels=FAKE, n=100, C=3, M=3, seed=1, r0=0, R=4, strat=0, work=FAKE, wb=BIG, conf=FAKE, u2=FAKE, npos=FAKE)
BOOT_INVALID = {
    "n_zero": dict(n=0), "n_negative": dict(n=-1), "n_32769": dict(n=32769, ms=32769 * 3), "C_zero": dict(C=0), "C_65": dict(C=65, ld=65, ms=6500),
    "M_zero": dict(M=0), "M_9": dict(M=9), "R_zero": dict(R=0), "R_negative": dict(R=-3), "r0_negative": dict(r0=-1),
    "r_past_2_31": dict(r0=(1 << 31) - 2, R=4), "work_bytes_small": dict(wb=1024), "work_bytes_one_short": dict(wb=None),
    "scores_null": dict(scores=None), "labels_null": dict(labels=None), "work_null": dict(work=None), "work_unaligned": dict(work=FAKE + 4),
    "nothing_to_compute": dict(conf=None, u2=None, npos=None), "u2_without_npos": dict(npos=None), "npos_without_u2": dict(u2=None),
    "ld_below_C": dict(ld=2), "models_overlap": dict(ms=299), "stratified_2": dict(strat=2),
}


def _boot_call(**kw):
    a = dict(BOOT_OK, **kw)
    h = _lib().lib()
    if a["wb"] is None:
        a["wb"] = h.mfvit_boot_work_bytes(a["n"], a["C"], a["M"], a["R"]) - 1
    return h.mfvit_boot_counts(a["scores"], a["ld"], a["ms"], a["labels"], a["n"], a["C"], a["M"], a["seed"], a["r0"], a["R"], a["strat"], a["work"],
                               a["wb"], a["conf"], a["u2"], a["npos"], None)


@pytest.mark.parametrize("case", sorted(BOOT_INVALID))
def test_boot_counts_refuses_invalid_calls_without_a_device(case):
    assert _boot_call(**BOOT_INVALID[case]) == EINVAL


DELONG_INVALID = {
    "n_zero": dict(n=0), "n_32769": dict(n=32769, ms=32769 * 3), "C_zero": dict(C=0), "C_65": dict(C=65, ld=65, ms=6500), "M_zero": dict(M=0),
    "M_9": dict(M=9), "work_bytes_small": dict(wb=1024), "work_bytes_one_short": dict(wb=None), "scores_null": dict(scores=None),
    "labels_null": dict(labels=None), "work_null": dict(work=None), "pos_xy_null": dict(pos_xy=None), "neg_xy_null": dict(neg_xy=None),
    "u2_null": dict(u2=None), "npos_null": dict(npos=None), "ld_below_C": dict(ld=2),
}


@pytest.mark.parametrize("case", sorted(DELONG_INVALID))
def test_delong_counts_refuses_invalid_calls_without_a_device(case):
    a = dict(scores=FAKE, ld=3, ms=300, labels=FAKE, n=100, C=3, M=3, work=FAKE, wb=BIG, v2=None, pos_xy=FAKE, neg_xy=FAKE, u2=FAKE, npos=FAKE)
    a.update(DELONG_INVALID[case])
    h = _lib().lib()
    if a["wb"] is None:
        a["wb"] = h.mfvit_boot_work_bytes(a["n"], a["C"], a["M"], 1) - 1
    assert h.mfvit_delong_counts(a["scores"], a["ld"], a["ms"], a["labels"], a["n"], a["C"], a["M"], a["work"], a["wb"], a["v2"], a["pos_xy"],
                                 a["neg_xy"], a["u2"], a["npos"], None) == EINVAL


def test_wrapper_argument_errors_come_before_any_launch():
    import torch
    es, Err = _es(), _lib().MfvitError
    s, t = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    for call in (lambda: es.bootstrap_counts(s, t, 10), lambda: es.delong(s, t), lambda: es.bootstrap_ci(s, t, n_boot=0),
                 lambda: es.bootstrap_ci(s, t, level=1.0), lambda: es.delong(s, t, level=0.0), lambda: es.PairedMeter([], 3),
                 lambda: es.PairedMeter(["a", "a"], 3), lambda: es.PairedMeter(list("abcdefghi"), 3), lambda: es.PairedMeter(["a"], 3).gathered(),
                 lambda: es.PairedMeter(["a", "b"], 3).update({"a": s}, t), lambda: es.PairedMeter(["a"], 4).update({"a": s}, t)):
        with pytest.raises(Err):
            call()


# ------------------------------------------------------------------------------------------------------- the host arithmetic
def test_statistics_on_a_hand_made_confusion_matrix():
    es = _es()
    conf = np.array([[[[5, 1, 0], [2, 3, 0], [0, 0, 0]]]], dtype=np.int64)                 # class 2 never occurs and is never predicted
    u2 = np.array([[[40, 30, 0]]], dtype=np.int64)
    npos = np.array([[6, 5, 0]], dtype=np.int64)
    st = es.stats_from_counts(conf, u2, npos, 11)
    assert st["accuracy"][0, 0] == 8 / 11
    np.testing.assert_allclose(st["precision"][0, 0], [5 / 7, 3 / 4, 0.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(st["recall"][0, 0], [5 / 6, 3 / 5, 0.0], rtol=0, atol=1e-15)
    f = [2 * (5 / 7) * (5 / 6) / (5 / 7 + 5 / 6), 2 * (3 / 4) * (3 / 5) / (3 / 4 + 3 / 5), 0.0]
    np.testing.assert_allclose(st["f1"][0, 0], f, rtol=0, atol=1e-15)
    assert abs(st["macro_f1"][0, 0] - sum(f) / 3) < 1e-15
    np.testing.assert_allclose(st["auc"][0, 0][:2], [40 / 60, 30 / 60], rtol=0, atol=1e-15)
    assert np.isnan(st["auc"][0, 0, 2]) and np.isnan(st["macro_auc"][0, 0])
    want = E.stats_of(conf[0, 0], u2[0, 0], npos[0], 11)
    for k, v in want.items():
        np.testing.assert_allclose(st[k][0, 0], v, rtol=0, atol=1e-15, equal_nan=True, err_msg=k)


def test_quantiles_and_p_values_on_hand_made_replicates():
    es = _es()
    v = np.array([0.1, 0.5, np.nan, 0.3, 0.2, 0.4])
    lo, hi, dropped = es.percentile_interval(v, 0.5)
    assert (float(lo), float(hi), int(dropped)) == (0.2, 0.4, 1)                         # quartiles of .1 .2 .3 .4 .5
    assert E.interval(v, 0.5) == (0.2, 0.4, 1)
    lo, hi, dropped = es.percentile_interval(np.full((3, 2), np.nan), 0.9)
    assert np.isnan(lo).all() and np.isnan(hi).all() and dropped.tolist() == [3, 3]
    d = np.array([[0.1, -0.2, 0.0], [0.2, -0.1, 0.0], [0.3, np.nan, 0.0], [-0.1, -0.3, np.nan]])
    p, used = es.bootstrap_p_value(d)
    assert used.tolist() == [4, 3, 3]
    np.testing.assert_allclose(p, [2 * 2 / 5, 2 * 1 / 4, 1.0], rtol=0, atol=1e-15)       # column 2: every delta 0 -> 2 * 4 / 4 capped at 1
    for j in range(3):
        assert E.p_two_sided(d[:, j]) == (float(p[j]), int(used[j]))
    p, used = es.bootstrap_p_value(np.full(4, np.nan))
    assert np.isnan(p) and used == 0


def test_summarize_from_integer_arrays_against_the_reference_end_to_end():
    """bootstrap_ci's host half on reference counts: points from replicate 0, intervals and p-values from the others, NaN replicates dropped"""
    es = _es()
    n, C, M, R = 40, 3, 2, 60
    rng = np.random.Generator(np.random.PCG64(3))
    t = rng.choice(C, size=n, p=[0.7, 0.25, 0.05]).astype(np.int64)                       # class 2 vanishes from some replicates
    s = rng.standard_normal((M, n, C)).astype(np.float32)
    s[0, np.arange(n), t] += 1.0
    conf, u2, npos = E.boot_counts(s, t, seed=5, r0=0, R=R + 1, brute=False)
    res = es.summarize(conf, u2, npos, n, level=0.9, names=["a", "b"])
    per = [[E.stats_of(conf[r, m], u2[r, m], npos[r], n) for m in range(M)] for r in range(R + 1)]
    assert res.models["a"]["macro_auc"].dropped > 0 and res.n_boot == R
    for m, nm in enumerate(["a", "b"]):
        for k in per[0][0]:
            got = res.models[nm][k]
            vals = np.array([per[r][m][k] for r in range(R + 1)], dtype=np.float64)
            cols = vals.reshape(R + 1, -1)
            want = [E.interval(cols[1:, j], 0.9) for j in range(cols.shape[1])]
            np.testing.assert_allclose(np.ravel(got.point), cols[0], rtol=0, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(np.ravel(got.lo), [x[0] for x in want], rtol=0, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(np.ravel(got.hi), [x[1] for x in want], rtol=0, atol=1e-12, equal_nan=True)
            assert np.ravel(got.dropped).tolist() == [x[2] for x in want]
    for k in per[0][0]:
        got = res.pairs[("a", "b")][k]
        d = (np.array([per[r][0][k] for r in range(R + 1)], dtype=np.float64) - np.array([per[r][1][k] for r in range(R + 1)])).reshape(R + 1, -1)
        want_p = [E.p_two_sided(d[1:, j]) for j in range(d.shape[1])]
        np.testing.assert_allclose(np.ravel(got.p), [x[0] for x in want_p], rtol=0, atol=1e-12, equal_nan=True)
        assert np.ravel(got.used).tolist() == [x[1] for x in want_p]
        np.testing.assert_allclose(np.ravel(got.point), d[0], rtol=0, atol=1e-12, equal_nan=True)
        rev = res.pairs[("b", "a")][k]
        np.testing.assert_allclose(np.ravel(rev.lo), -np.ravel(got.hi), rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_array_equal(np.ravel(rev.p), np.ravel(got.p))                       # two-sided: the same either way round
