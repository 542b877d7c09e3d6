"""GPU: the curve of the sample, operating points of bootstrap replicates and calibration sums (csrc/evalstats.hip: curve_kernel, points_kernel,
calib_kernel) through the C ABI inside guarded buffers and through mfvit.evalstats, every integer and every threshold bit for bit against
tests/opcurve_ref.py, at the sizes where the shared loops turn over (the order kernel's 256-sample block and 1,024-key chunk, the 512-place scan
tile, each minus one, exact and plus one) and at the LDS-heaviest shape."""
import math

import numpy as np
import pytest
import torch

import evalstats_ref as E
import opcurve_ref as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -22
N_EDGES = (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
KINDS = ("gauss", "ties", "equal", "special")
LKINDS = ("random", "outside", "missing")
EXTRA, PADROWS, GUARD = 3, 2, 8
FILL = {torch.int64: -0x0123456789ABCDEF, torch.int32: -0x01234567, torch.float32: -19088744.0,torch.float64: -81985529216486895.0}
U = 2.0 ** -53
# The accuracy of the device's double exp / log is stated nowhere in the ROCm documentation that ships with the toolchain, so it was MEASURED:
# tools/perf_opcurve.py runs mfvit_calib_sums with one row per workgroup (no summation at all) over 61,440 (row, temperature) terms and records
# the worst |device - restatement| / (1 + the magnitude of the term's parts), and the worst relative error of a confidence, in
# profiles/opcurve_bench.txt: 6.78 U (its line "worst single-row error").  The gate allows 4 times that per row on top of the summation
# order's share.
TERM_ERR = 4 * 6.78 * U
CAL_T = 256                                # threads of a calibration workgroup: a thread's chain holds ceil(n / 256) rows, the tree 8 levels


def _guarded(numel, dtype):
    buf = torch.full((GUARD + numel + GUARD,), FILL[dtype], device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + numel]


def _intact(g):
    buf, _ = g
    fill = FILL[buf.dtype]
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _untouched(g):
    return bool((g[0] == FILL[g[0].dtype]).all())


def _layout(scores):
    """scores [M, n, C] as the slice wide[:, :n, :C] of a NaN-filled [M, n + PADROWS, C + EXTRA] tensor: ld = C + 3 and a padded model stride"""
    M, n, C = scores.shape
    wide = torch.full((M, n + PADROWS, C + EXTRA), float("nan"), device=DEV)
    wide[:, :n, :C] = torch.from_numpy(scores).to(DEV)
    return wide, wide[:, :n, :C]


def _curve(scores, labels):
    from mfvit._lib import check, lib, ptr, stream
    M, n, C = scores.shape
    wide, view = _layout(scores)
    lab = torch.from_numpy(labels).to(DEV)
    wide0 = wide.clone()
    thr, tp, fp = _guarded(M * C * n, torch.float32), _guarded(M * C * n, torch.int32), _guarded(M * C * n, torch.int32)
    nthr, nnan, npos = _guarded(M * C, torch.int32), _guarded(M * C, torch.int32), _guarded(C, torch.int64)
    nbytes = lib().mfvit_boot_work_bytes(n, C, M, 1)
    work = torch.full((nbytes + 256,), 0xA5, device=DEV, dtype=torch.uint8)
    check(lib().mfvit_curve_counts(ptr(view), view.stride(1), view.stride(0), ptr(lab), n, C, M, ptr(work), nbytes, ptr(thr[1]), ptr(tp[1]), ptr(fp[1]),
                                   ptr(nthr[1]), ptr(nnan[1]), ptr(npos[1]), stream()), "mfvit_curve_counts")
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int32), wide0.view(torch.int32))                                     # inputs are read-only
    assert all(_intact(g) for g in (thr, tp, fp, nthr, nnan, npos)) and bool((work[nbytes:] == 0xA5).all())
    return (thr[1].view(M, C, n).cpu().numpy(), tp[1].view(M, C, n).cpu().numpy().astype(np.int64), fp[1].view(M, C, n).cpu().numpy().astype(np.int64),
            nthr[1].view(M, C).cpu().numpy().astype(np.int64), nnan[1].view(M, C).cpu().numpy().astype(np.int64), npos[1].cpu().numpy())


def _points(scores, labels, seed, r0, R, stratified, req):
    from mfvit._lib import check, lib, ptr, stream
    M, n, C = scores.shape
    req = np.ascontiguousarray(req, dtype=np.int32).reshape(-1, 3)
    Q = req.shape[0]
    wide, view = _layout(scores)
    lab = torch.from_numpy(labels).to(DEV)
    rq = torch.from_numpy(req).to(DEV)
    wide0, rq0 = wide.clone(), rq.clone()
    tp, fp, thr = _guarded(R * M * C * Q, torch.int32), _guarded(R * M * C * Q, torch.int32), _guarded(R * M * C * Q, torch.float32)
    npos = _guarded(R * C, torch.int64)
    nbytes = lib().mfvit_boot_work_bytes(n, C, M, R)
    work = torch.full((nbytes + 256,), 0xA5, device=DEV, dtype=torch.uint8)
    check(lib().mfvit_boot_points(ptr(view), view.stride(1), view.stride(0), ptr(lab), n, C, M, seed, r0, R, int(stratified), ptr(rq), Q, ptr(work), nbytes,
                                  ptr(tp[1]), ptr(fp[1]), ptr(thr[1]), ptr(npos[1]), stream()), "mfvit_boot_points")
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int32), wide0.view(torch.int32)) and torch.equal(rq, rq0)
    assert all(_intact(g) for g in (tp, fp, thr, npos)) and bool((work[nbytes:] == 0xA5).all())
    sh = (R, M, C, Q)
    return (tp[1].view(sh).cpu().numpy().astype(np.int64), fp[1].view(sh).cpu().numpy().astype(np.int64), thr[1].view(sh).cpu().numpy(),
            npos[1].view(R, C).cpu().numpy())


def _calib(logits, labels, temps, NB):
    import ctypes
    from mfvit._lib import check, lib, ptr, stream
    M, n, C = logits.shape
    t32 = np.ascontiguousarray(temps, dtype=np.float32)
    Kt = t32.size
    wide, view = _layout(logits)
    lab = torch.from_numpy(labels).to(DEV)
    wide0 = wide.clone()
    bn, bh = _guarded(M * Kt * NB, torch.int64), _guarded(M * Kt * NB, torch.int64)
    bc, sm, sk = _guarded(M * Kt * NB, torch.float64), _guarded(M * Kt * 3, torch.float64), _guarded(M, torch.int64)
    check(lib().mfvit_calib_sums(ptr(view), view.stride(1), view.stride(0), ptr(lab), n, C, M, t32.ctypes.data_as(ctypes.c_void_p), Kt, NB, ptr(bn[1]),
                                 ptr(bh[1]), ptr(bc[1]), ptr(sm[1]), ptr(sk[1]), stream()), "mfvit_calib_sums")
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int32), wide0.view(torch.int32)) and all(_intact(g) for g in (bn, bh, bc, sm, sk))
    return dict(bin_n=bn[1].view(M, Kt, NB).cpu().numpy(), bin_hit=bh[1].view(M, Kt, NB).cpu().numpy(), bin_conf=bc[1].view(M, Kt, NB).cpu().numpy(),
                sums=sm[1].view(M, Kt, 3).cpu().numpy(), skipped=sk[1].cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_curve(got, want, what):
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=f"thr {what}")      # NaN past nthr: the same quiet NaN, bit for bit
    for g, w, name in zip(got[1:], want[1:], ("tp", "fp", "nthr", "nnan", "npos")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def _same_points(got, want, what):
    for g, w, name in zip(got, want, ("tp", "fp", "thr", "npos")):
        if name == "thr":
            g, w = _bits(g), _bits(w)
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def _requests(s, rng, Q):
    """Q requests that start with the extremes: a = 0 and a = b of both rational kinds, a tau above every score, below every score, on a tied
    (or any held) value, NaN; then random fractions and thresholds"""
    held = s[~np.isnan(s)]
    tied = float(np.sort(held)[held.size // 2]) if held.size else 0.0
    at = [("specificity", 1.0), ("specificity", 0.0), ("sensitivity", 0.0), ("sensitivity", 1.0), ("threshold", float("inf")),
          ("threshold", float("-inf")), ("threshold", tied), ("threshold", float("nan")), ("threshold", 3.0e38), ("threshold", -3.0e38),
          ("specificity", 0.95), ("sensitivity", 0.9), ("specificity", 1 / 3), ("sensitivity", 2 / 3)]
    while len(at) < Q:
        k = len(at) % 3
        at.append((("specificity", "sensitivity", "threshold")[k], float(rng.random()) if k < 2 else float(np.float32(rng.standard_normal()))))
    if Q < len(at):
        at = [at[int(i)] for i in rng.permutation(len(at))[:Q]]
    return O.request_rows(at)


# ------------------------------------------------------------------------------------------------------- curve and points, bit for bit
@pytest.mark.parametrize("n", N_EDGES)
def test_curve_and_points_bit_exact_at_block_chunk_and_tile_edges(n):
    i = N_EDGES.index(n)
    M, C, R = (1, 2)[i % 2], 2, 3
    rng = np.random.Generator(np.random.PCG64(n))
    for k, kind in enumerate(KINDS):
        lkind, strat = LKINDS[(i + k) % 3], (i + k) % 2 == 1
        s, t = E.case(n, C, M, kind, lkind, 13 * n + k)
        _same_curve(_curve(s, t), O.curve_counts(s, t), (n, kind, lkind))
        req = _requests(s, rng, 14)
        _same_points(_points(s, t, 500 + n, 0, R, strat, req), O.boot_points(s, t, 500 + n, 0, R, strat, req), (n, kind, lkind, strat))


def test_curve_and_points_at_the_largest_sample_count():
    """n = 32768: both prefixes of a column share 128 KiB of LDS, a prefix half may reach 2^15"""
    n, C = 32768, 2
    s, t = E.case(n, C, 1, "ties", "random", 99)
    s[0, 100:140, 0] = np.nan
    _same_curve(_curve(s, t), O.curve_counts(s, t), "n = 32768")
    req = _requests(s, np.random.Generator(np.random.PCG64(1)), 14)
    for strat in (False, True):
        _same_points(_points(s, t, (7 << 32) + 5, 0, 3, strat, req), O.boot_points(s, t, (7 << 32) + 5, 0, 3, strat, req), ("n = 32768", strat))
    one = np.zeros((1, n, 1), dtype=np.float32)                          # one tie group, every sample a positive: the low half reaches 32768
    lab = np.zeros(n, dtype=np.int64)
    _same_curve(_curve(one, lab), O.curve_counts(one, lab), "all equal, all positive")
    _same_points(_points(one, lab, 3, 0, 2, False, req), O.boot_points(one, lab, 3, 0, 2, False, req), "all equal, all positive")
    _same_points(_points(one, lab - 1, 3, 0, 2, False, req), O.boot_points(one, lab - 1, 3, 0, 2, False, req), "all equal, all negative")


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("C", [1, 2, 3, 64])
def test_class_model_and_request_counts(C, M):
    n, R = 40, 2
    rng = np.random.Generator(np.random.PCG64(100 * C + M))
    for kind, lkind, strat, Q in (("special", "outside", True, 64), ("ties", "missing", False, 1)):
        s, t = E.case(n, C, M, kind, lkind, 10 * C + M)
        _same_curve(_curve(s, t), O.curve_counts(s, t), (C, M, kind))
        req = _requests(s, rng, Q)
        _same_points(_points(s, t, C, 0, R, strat, req), O.boot_points(s, t, C, 0, R, strat, req), (C, M, kind, Q))


def test_denormals_zero_signs_infinities_and_requests_that_are_none():
    n, C, M = 300, 2, 2
    rng = np.random.Generator(np.random.PCG64(4))
    pool = np.array([1e-45, -1e-45, 3e-45, 0.0, -0.0, 1e-40, -1e-40, 1.1754944e-38, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32)
    s = pool[rng.integers(0, pool.size, (M, n, C))]
    _, t = E.case(n, C, M, "gauss", "outside", 5)
    got = _curve(s, t)
    _same_curve(got, O.curve_counts(s, t), "denormals")
    assert (got[3] == 11).all()                                           # eleven distinct numbers: the denormals keep their order, the zeros are one
    at = [("threshold", float(v)) for v in pool] + [("specificity", 0.9), ("sensitivity", 0.9)]
    req = np.concatenate([O.request_rows(at), np.array([[3, 1, 2], [-1, 0, 1], [0, 2, 1], [1, -1, 4], [0, 1, 0], [1, 1, (1 << 20) + 1]], dtype=np.int32)])
    tp, fp, thr, npos = _points(s, t, 9, 0, 3, False, req)
    k = len(at)
    _same_points((tp[..., :k], fp[..., :k], thr[..., :k], npos), O.boot_points(s, t, 9, 0, 3, False, req[:k]), "denormals")
    assert not tp[..., k:].any() and not fp[..., k:].any() and np.isnan(thr[..., k:]).all()          # not a request: 0, 0, NaN


def test_replicates_without_positives_or_negatives():
    for labels, strat in ((np.array([0, 0, 1], dtype=np.int64), False), (np.array([0, 0, 0], dtype=np.int64), True),
                          (np.array([1, 0, 7], dtype=np.int64), False)):
        n, C, M, R = 3, 2, 2, 40
        s, _ = E.case(n, C, M, "ties", "random", 3)
        req = _requests(s, np.random.Generator(np.random.PCG64(2)), 14)
        want = O.boot_points(s, labels, 21, 0, R, strat, req)
        assert (want[3] == 0).any() and (want[3] == n).any()              # P_r = 0 and N_r = 0 both occur
        _same_points(_points(s, labels, 21, 0, R, strat, req), want, (labels.tolist(), strat))


def test_replicate_zero_at_every_threshold_is_the_curve_and_npos_is_boot_counts():
    from mfvit._lib import check, lib, ptr, stream
    n, C, M = 60, 2, 2
    s, t = E.case(n, C, M, "special", "outside", 8)
    thr, tp, fp, nthr, _, _ = _curve(s, t)
    for m in range(M):
        for c in range(C):
            G = int(nthr[m, c])
            assert 0 < G <= 64
            req = np.array([(2, int(_bits(thr[m, c, k:k + 1])[0]), 0) for k in range(G)], dtype=np.int32)
            btp, bfp, bthr, _ = _points(s, t, 1, 0, 1, False, req)
            np.testing.assert_array_equal(btp[0, m, c], tp[m, c, :G])
            np.testing.assert_array_equal(bfp[0, m, c], fp[m, c, :G])
            np.testing.assert_array_equal(_bits(bthr[0, m, c]), _bits(thr[m, c, :G]))
    R, seed = 6, 0xFEDCBA9876543210
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    for strat in (False, True):
        u2 = torch.empty(R, M, C, device=DEV, dtype=torch.int64)
        npos = torch.empty(R, C, device=DEV, dtype=torch.int64)
        nbytes = lib().mfvit_boot_work_bytes(n, C, M, R)
        work = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
        check(lib().mfvit_boot_counts(ptr(sd), C, n * C, ptr(td), n, C, M, seed, 2, R, int(strat), ptr(work), nbytes, None, ptr(u2), ptr(npos), stream()),
              "mfvit_boot_counts")
        np.testing.assert_array_equal(_points(s, t, seed, 2, R, strat, np.array([[0, 1, 20]]))[3], npos.cpu().numpy())


def test_replicates_are_absolute_and_calls_repeat_their_bits():
    n, C, M = 700, 3, 2
    s, t = E.case(n, C, M, "ties", "outside", 4)
    req = _requests(s, np.random.Generator(np.random.PCG64(3)), 14)
    seed = 0xFEDCBA9876543210
    for strat in (False, True):
        whole = _points(s, t, seed, 0, 7, strat, req)
        _same_points(_points(s, t, seed, 0, 7, strat, req), whole, "the same call again")
        parts = [_points(s, t, seed, r0, R, strat, req) for r0, R in ((0, 2), (2, 4), (6, 1))]
        _same_points([np.concatenate([p[k] for p in parts]) for k in range(4)], whole, "chunks")
    _same_points(_points(s, t, seed, 123456, 2, False, req), O.boot_points(s, t, seed, 123456, 2, False, req), "r0 = 123456")


def test_points_past_the_replicates_of_one_launch():
    """the library launches 65,536 replicates at a time: replicates 65,534 .. 65,539 of one call lie on both sides of that turn-over"""
    n, C, M, R = 9, 2, 1, 65540
    s, t = E.case(n, C, M, "ties", "random", 3)
    req = O.request_rows([("specificity", 0.75), ("sensitivity", 0.5), ("threshold", 0.0)])
    got = _points(s, t, 11, 0, R, True, req)
    for r0, k in ((0, 3), (65534, 6)):
        _same_points([g[r0:r0 + k] for g in got], O.boot_points(s, t, 11, r0, k, True, req), r0)


# ------------------------------------------------------------------------------------------------------- calibration
def _logit_case(n, C, M, seed, scale=3.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    z = (scale * rng.standard_normal((M, n, C))).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.int64)
    return z, y


def _check_calib(z, y, temps, NB, what):
    """counts exact (every confidence at least 1e-9 from a bin edge, asserted, no row left out); the double sums within the gate"""
    M, n, C = z.shape
    ref = O.calib_sums(z, y, temps, NB)
    assert NB == 1 or O.edge_margin(ref["conf"], NB) >= 1e-9, (what, "pick another seed: a confidence lies on a bin edge")
    got = _calib(z, y, temps, NB)
    for k in ("bin_n", "bin_hit", "skipped"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} {what}")
    # The restatement's sums are correctly rounded (math.fsum), so the gate is the device's share alone.  Summation order: a thread's chain of
    # ceil(n / 256) rows, then 8 tree levels (the bins: 3 adds and 6 levels, fewer), times U, times the sum of the magnitudes.  Per row TERM_ERR,
    # relative to 1 + the magnitude of the row's parts (the 1: what cancellation leaves of the absolute rounding of den and p_y).
    order = (math.ceil(n / CAL_T) + 8) * U
    used = (n - ref["skipped"])[:, None, None]
    gate = order * ref["abs_sums"] + TERM_ERR * (used + ref["abs_sums"])
    err = np.abs(got["sums"] - ref["sums"])
    print(f"{what}: worst sums error / gate = {np.max(err / np.maximum(gate, 1e-300)):.3f}; worst error / (rows + magnitude sum) = "
          f"{np.max(err / np.maximum(used + ref['abs_sums'], 1e-300)) / U:.2f} U")
    assert (err <= gate).all(), (what, err, gate)
    berr = np.abs(got["bin_conf"] - ref["bin_conf"])
    print(f"{what}: worst bin_conf error / bin sum = {np.max(berr / np.maximum(ref['bin_conf'], 1e-300)) / U:.2f} U, gate {(order + TERM_ERR) / U:.1f} U")
    assert (berr <= (order + TERM_ERR) * ref["bin_conf"]).all(), (what, berr)
    return got, ref


@pytest.mark.parametrize("NB", [1, 15, 64])
@pytest.mark.parametrize("Kt", [1, 16])
def test_calibration_sums_bins_and_temperatures(Kt, NB):
    temps = np.float32(0.25 * 1.35 ** np.arange(Kt)) if Kt > 1 else np.float32([1.0])
    for n, C, M in ((1000, 3, 2), (257, 5, 1), (1, 2, 8)):
        z, y = _logit_case(n, C, M, 1000 * Kt + NB + n)
        _check_calib(z, y, temps, NB, (n, C, M, Kt, NB))


@pytest.mark.parametrize("kind", KINDS)
def test_calibration_on_the_score_kinds(kind):
    """the cases of the curve tests as logits: heavy ties and all-equal rows (the first maximum decides the top label), rows with NaN / +-inf
    (skipped), labels outside the classes (skipped) and a missing class.  One bin where equal logits put confidences ON inner edges (1 / 2, 1 / 3)."""
    for n, C, M, lkind, NB in ((300, 3, 2, "outside", 1), (513, 4, 1, "missing", 1 if kind in ("equal", "special", "ties") else 15)):
        z, y = E.case(n, C, M, kind, lkind, 7 * n + C)
        got, ref = _check_calib(z, y, np.float32([0.5, 1.0, 3.0]), NB, (kind, lkind, NB))
        assert kind != "special" or (ref["skipped"] > n // 10).all()
        assert (got["bin_n"].sum(2) == (n - ref["skipped"])[:, None]).all()


def test_calibration_edge_values():
    n, C, M = 600, 3, 2
    z, y = _logit_case(n, C, M, 12)
    z[0, 5, 1], z[0, 6, 0], z[1, 7, 2], z[1, 8, 1] = np.inf, -np.inf, np.nan, np.inf
    y[9], y[10], y[11] = -1, C, 2 ** 32
    z[:, 20] = (300.0, -300.0, 0.0)                                      # saturated: confidence exactly 1, the last bin
    got, ref = _check_calib(z, y, np.float32([0.5, 1.0, 4.0]), 15, "edge values")
    assert got["skipped"].tolist() == [5, 5] and ref["conf"][0, 1, 20] == 1.0
    z1, y1 = np.zeros((1, 300, 1), dtype=np.float32), np.zeros(300, dtype=np.int64)
    z1[0, :, 0] = np.linspace(-5, 5, 300)
    got, _ = _check_calib(z1, y1, np.float32([0.1, 2.0]), 7, "one class")
    assert (got["bin_n"][0, :, 6] == 300).all() and (got["sums"] == 0.0).all() and (got["bin_conf"][0, :, 6] == 300.0).all()
    big, yb = _logit_case(32768, 3, 1, 77)
    _check_calib(big, yb, np.float32([1.0, 2.0]), 15, "n = 32768")
    a, b = _calib(big, yb, np.float32([1.0, 2.0]), 15), _calib(big, yb, np.float32([1.0, 2.0]), 15)
    assert all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)             # the same bits on every call


# ------------------------------------------------------------------------------------------------------- end to end
def _three_streams(n, C, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = rng.choice(C, size=n, p=[0.6, 0.3, 0.1]).astype(np.int64)
    fus, cxr, enh = (np.round(rng.standard_normal((n, C)) * 16).astype(np.float32) / 16 for _ in range(3))
    for k, x in enumerate((fus, cxr, enh)):
        x[np.arange(n), t] += 0.5 + 0.25 * k
    return fus, cxr, enh, t


def test_paired_meter_operating_points_over_ragged_batches():
    from mfvit import evalstats
    n, C, n_boot = 700, 3, 30
    fus, cxr, enh, t = _three_streams(n, C, 21)
    names = ["sum", "cxr", "enh"]
    meter = evalstats.PairedMeter(names, C)
    i = 0
    for bs in (256, 1, 255, 188):
        f, c, e = (torch.from_numpy(x[i:i + bs]).to(DEV) for x in (fus, cxr, enh))
        meter.update({"sum": f + c + e, "cxr": c, "enh": e}, torch.from_numpy(t[i:i + bs]).to(DEV).float())
        i += bs
    scores = np.stack([(torch.from_numpy(fus) + torch.from_numpy(cxr) + torch.from_numpy(enh)).numpy(), cxr, enh])
    at = [("specificity", 0.95), ("sensitivity", 0.9), ("threshold", 0.5)]
    for strat in (False, True):
        op = meter.operating_points(at, n_boot=n_boot, level=0.9, seed=77, stratified=strat)
        tp, fp, thr, npos = O.boot_points(scores, t, 77, 0, n_boot + 1, strat, O.request_rows(at))
        want = evalstats.summarize_points(tp, fp, thr, npos, n, at, 0.9, names)          # the host arithmetic is pinned in test_opcurve_cpu.py
        assert op.names == names and op.n_boot == n_boot and op.at == at
        for nm in names:
            np.testing.assert_array_equal(_bits(op.models[nm]["threshold"]), _bits(want.models[nm]["threshold"]))
            for k in evalstats.POINT_STATS:
                for g, w in zip(op.models[nm][k], want.models[nm][k]):
                    np.testing.assert_array_equal(g, w, err_msg=f"{nm} {k} {strat}")
        for pair, stats in want.pairs.items():
            for k, w in stats.items():
                for g, x in zip(op.pairs[pair][k], w):
                    np.testing.assert_array_equal(g, x, err_msg=f"{pair} {k} {strat}")
        # sensitivity at 95 % specificity by hand for the sample itself: the lowest threshold with FP <= floor(N / 20)
        c, s0 = 0, scores[0, :, 0]
        cap = int((t != c).sum()) // 20
        cand = np.unique(s0)[::-1]
        ok = [v for v in cand if ((s0 >= v) & (t != c)).sum() <= cap]
        assert op.models["sum"]["sensitivity"].point[c, 0] == ((s0 >= ok[-1]) & (t == c)).sum() / (t == c).sum()
    sd, td = torch.from_numpy(scores).to(DEV), torch.from_numpy(t).to(DEV)
    whole = evalstats.bootstrap_points(sd, td, O.request_rows(at), 10, seed=3)
    for chunk in (1, 4, 11, 1000):
        for g, w in zip(evalstats.bootstrap_points(sd, td, O.request_rows(at), 10, seed=3, chunk=chunk), whole):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
    band = evalstats.roc_band(sd, td, n_boot=20, seed=5, names=names)
    op = evalstats.operating_points(sd, td, [("specificity", k / 20) for k in range(21)], n_boot=20, seed=5, names=names)
    assert band.fpr.shape == (21,) and band.tpr["sum"].shape == (C, 21)
    np.testing.assert_array_equal(band.lo["cxr"], op.models["cxr"]["sensitivity"].lo)
    assert (band.lo["sum"] <= band.tpr["sum"] + 1e-12).any() and (band.tpr["sum"][:, 0] == 1.0).all()      # specificity 0: everything predicted positive


def test_epoch_meter_curves_calibration_and_temperature():
    from sklearn import metrics as skm
    from mfvit import evalstats, metrics
    n, C = 500, 3
    _, cxr, _, t = _three_streams(n, C, 8)
    sd, td = torch.from_numpy(cxr).to(DEV), torch.from_numpy(t).to(DEV)
    meter = metrics.EpochMeter(C)
    meter.update(sd[:300], td[:300].float(), torch.zeros((), device=DEV))
    meter.update(sd[300:], td[300:].float(), torch.zeros((), device=DEV))
    roc = meter.roc_curve()
    pr, ap = evalstats.precision_recall_curve(sd, td), evalstats.average_precision(sd, td)
    for c in range(C):
        fpr, tpr, thresholds = skm.roc_curve(t == c, cxr[:, c])
        np.testing.assert_array_equal(roc[c].fpr, fpr)
        np.testing.assert_array_equal(roc[c].tpr, tpr)
        np.testing.assert_array_equal(_bits(roc[c].thresholds), _bits(thresholds))
        prec, rec, _ = skm.precision_recall_curve(t == c, cxr[:, c])
        np.testing.assert_array_equal(pr[c].precision, prec)
        np.testing.assert_array_equal(pr[c].recall, rec)
        assert abs(ap[c] - skm.average_precision_score(t == c, cxr[:, c])) <= (2 * n + 16) * U       # the bound derived in test_opcurve_cpu.py
    op = meter.operating_points([("specificity", 0.9)], n_boot=20, seed=1)
    assert op.names == ["0"] and op.models["0"]["sensitivity"].point.shape == (C, 1)
    bad = cxr.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        evalstats.roc_curve(torch.from_numpy(bad).to(DEV), td)
    # calibration: the meter's outputs as logits
    cal = meter.calibration(temperature=1.5, n_bins=10)
    ref = O.calib_sums(cxr, t, [1.5], 10)
    assert O.edge_margin(ref["conf"], 10) >= 1e-9
    want = evalstats.calibration_from_sums(ref["bin_n"][0, 0], ref["bin_hit"][0, 0], ref["bin_conf"][0, 0], ref["sums"][0, 0], 0, n, 1.5)
    np.testing.assert_array_equal(cal.bin_count, want.bin_count)
    np.testing.assert_array_equal(cal.bin_accuracy, want.bin_accuracy)
    tol = (math.ceil(n / CAL_T) + 8 + 16) * U                            # the gate of _check_calib on quantities <= 1 (the NLL: per row <= ~20)
    assert abs(cal.ece - want.ece) <= 4 * tol and abs(cal.mce - want.mce) <= 4 * tol and abs(cal.brier - want.brier) <= 2 * tol
    assert abs(cal.nll - want.nll) <= 20 * tol and cal.used == n and cal.skipped == 0
    direct = O.calibration_direct(cxr, t, 1.5, 10)
    assert abs(cal.ece - direct[0]) < 1e-12 and abs(cal.brier - direct[2]) < 1e-12 and abs(cal.nll - direct[3]) < 1e-12
    # temperature scaling: logits scaled by a known factor move the fitted temperature by that factor
    base = evalstats.fit_temperature(sd, td)
    lo, hi = evalstats.refine_bracket(lambda tt: O.calib_sums(cxr, t, tt, 1)["sums"][0, :, 2], 0.05, 20.0)
    assert lo - (hi - lo) <= base <= hi + (hi - lo), (base, lo, hi)       # the restatement's minimiser, within the bracket width
    for factor in (0.25, 4.0):                                            # powers of two: the scaled logits are exact
        got = evalstats.fit_temperature(sd * factor, td)
        assert abs(got - factor * base) <= 2e-6 * factor * base, (factor, got, base)
        assert got == evalstats.fit_temperature(sd * factor, td)          # repeats its bits
    assert evalstats.fit_temperature(sd, td, lo=5.0, hi=20.0) == 5.0     # the sign never changes: the bracket's end


# ------------------------------------------------------------------------------------------------------- refusals leave the outputs alone
def test_argument_errors_leave_the_guarded_outputs_untouched():
    import ctypes
    from mfvit._lib import lib, ptr, stream
    n, C, M, R, Q = 50, 3, 2, 3, 2
    s, t = E.case(n, C, M, "gauss", "random", 1)
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    rq = torch.from_numpy(O.request_rows([("specificity", 0.9), ("threshold", 0.0)])).to(DEV)
    L = lib()
    nbytes = L.mfvit_boot_work_bytes(n, C, M, R)
    work = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    outs = [_guarded(M * C * n, torch.float32), _guarded(M * C * n, torch.int32), _guarded(M * C * n, torch.int32), _guarded(M * C, torch.int32),
            _guarded(M * C, torch.int32), _guarded(C, torch.int64)]
    o = [ptr(g[1]) for g in outs]
    for a in ((ptr(sd), C - 1, n * C, ptr(td), n, C, M, ptr(work), nbytes), (ptr(sd), C, n * C - 1, ptr(td), n, C, M, ptr(work), nbytes),
              (ptr(sd), C, n * C, ptr(td), n, C, M, ptr(work), 16), (ptr(sd), C, n * C, ptr(td), n, 65, M, ptr(work), nbytes),
              (ptr(sd), C, n * C, ptr(td), 0, C, M, ptr(work), nbytes), (ptr(sd), C, n * C, ptr(td), n, C, 9, ptr(work), nbytes)):
        assert L.mfvit_curve_counts(*a, *o, stream()) == EINVAL
    outs2 = [_guarded(R * M * C * Q, torch.int32), _guarded(R * M * C * Q, torch.int32), _guarded(R * M * C * Q, torch.float32), _guarded(R * C, torch.int64)]
    o2 = [ptr(g[1]) for g in outs2]
    for r0, Rr, strat, q, wb in ((-1, R, 0, Q, nbytes), (0, 0, 0, Q, nbytes), (2 ** 31 - 2, R, 0, Q, nbytes), (0, R, 2, Q, nbytes), (0, R, 0, 0, nbytes),
                                 (0, R, 0, 65, nbytes), (0, R, 0, Q, nbytes - 1)):
        assert L.mfvit_boot_points(ptr(sd), C, n * C, ptr(td), n, C, M, 1, r0, Rr, strat, ptr(rq), q, ptr(work), wb, *o2, stream()) == EINVAL
    outs3 = [_guarded(M * 2 * 15, torch.int64), _guarded(M * 2 * 15, torch.int64), _guarded(M * 2 * 15, torch.float64), _guarded(M * 2 * 3, torch.float64),
             _guarded(M, torch.int64)]
    o3 = [ptr(g[1]) for g in outs3]
    for temps, Kt, NB in (([1.0, 0.0], 2, 15), ([1.0, -2.0], 2, 15), ([float("nan"), 1.0], 2, 15), ([float("inf"), 1.0], 2, 15), ([1.0, 1.0], 0, 15),
                          ([1.0] * 17, 17, 15), ([1.0, 1.0], 2, 0), ([1.0, 1.0], 2, 65)):
        arr = (ctypes.c_float * len(temps))(*temps)
        assert L.mfvit_calib_sums(ptr(sd), C, n * C, ptr(td), n, C, M, ctypes.cast(arr, ctypes.c_void_p), Kt, NB, *o3, stream()) == EINVAL
    torch.cuda.synchronize()
    assert all(_intact(g) and _untouched((g[1],)) for g in outs + outs2 + outs3)
