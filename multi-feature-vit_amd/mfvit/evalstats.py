"""How certain is an epoch's AUC, and is one score set significantly better than another on the same test set?

The reference's drivers report one number per metric (MAIN_CA:886-911, MAIN_SS:797-821).  This module adds bootstrap percentile intervals,
paired bootstrap tests and DeLong's test for the AUC.  The counting runs on the GPU (csrc/evalstats.hip: every (model, class) column is ordered
once, a replicate then costs O(n) per column); all device results are integers, copied to the host once, and the arithmetic on them is float64
(as EpochMeter.compute does it).

    ci = bootstrap_ci(torch.stack([out_fus + out_cxr + out_enh, out_cxr, out_enh]), target, names=["sum", "cxr", "enh"])
    ci.models["sum"]["macro_auc"]            # Interval(point, lo, hi, dropped)
    ci.pairs[("sum", "cxr")]["macro_auc"]    # PairInterval(point, lo, hi, p, used): delta = sum - cxr
    dl = delong(scores, target)              # dl.auc [M, C], dl.var, dl.lo, dl.hi, dl.cov [C, M, M], dl.z, dl.p

The curve itself and what a diagnostic study reads off it come from the same ordered columns (curve_kernel, points_kernel, calib_kernel):

    roc = roc_curve(scores, target)          # per class (fpr, tpr, thresholds) as scikit-learn; precision_recall_curve, average_precision
    op = operating_points(scores, target, [("specificity", 0.95), ("threshold", tau_val)], names=["sum", "cxr", "enh"])
    op.models["sum"]["sensitivity"]          # Interval with [C, Q] arrays;  op.pairs[("sum", "cxr")]["sensitivity"]: the paired difference
    cal = calibration(logits, target)        # cal.ece, cal.mce, cal.brier, cal.nll, the reliability diagram;  T = fit_temperature(logits, target)
"""
import math
from collections import namedtuple
from statistics import NormalDist

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, require_cuda, stream

MAX_N, MAX_C, MAX_M = 32768, 64, 8
WORK_BUDGET = 256 << 20            # bytes of scratch a bootstrap call may hold at a time: the replicates run in chunks that fit

Interval = namedtuple("Interval", "point lo hi dropped")            # dropped: replicates left out of the quantiles (the statistic was NaN)
PairInterval = namedtuple("PairInterval", "point lo hi p used")     # used: replicates behind the interval and the p-value
BootstrapResult = namedtuple("BootstrapResult", "names level n_boot models pairs")
DelongResult = namedtuple("DelongResult", "names level auc var lo hi cov z p npos n")


def _prepare(scores, labels):
    require_cuda(scores, labels)
    if scores.dim() == 2:
        scores = scores.unsqueeze(0)
    if scores.dim() != 3 or scores.dtype != torch.float32 or labels.dtype != torch.int64:
        raise _lib.MfvitError("evalstats wants float32 [n, C] or [M, n, C] scores and int64 labels")
    M, n, C = scores.shape
    if labels.dim() != 1 or labels.shape[0] != n:
        raise _lib.MfvitError("labels must be [n], one per score row")
    if not (1 <= n <= MAX_N and 1 <= C <= MAX_C and 1 <= M <= MAX_M):
        raise _lib.MfvitError(f"evalstats limits: 1 <= n <= {MAX_N}, 1 <= C <= {MAX_C}, 1 <= M <= {MAX_M}; got n = {n}, C = {C}, M = {M}")
    if scores.stride(2) != 1 or scores.stride(1) < C or (M > 1 and scores.stride(0) < (n - 1) * scores.stride(1) + C):
        scores = scores.contiguous()
    return scores, labels.contiguous(), M, n, C


def bootstrap_counts(scores, labels, n_boot, seed=0, stratified=False, chunk=None):
    """scores f32 [n, C] or [M, n, C], labels int64 [n] on the GPU -> (conf [n_boot + 1, M, C, C], u2 [n_boot + 1, M, C], npos [n_boot + 1, C]),
    int64 on the GPU; replicate 0 is the sample itself (include/mfvit.h, mfvit_boot_counts).  The result does not depend on `chunk`."""
    scores, labels, M, n, C = _prepare(scores, labels)
    if n_boot < 0 or not 0 <= seed < 1 << 64:
        raise _lib.MfvitError("n_boot must be >= 0 and the seed an unsigned 64-bit value")
    R = n_boot + 1
    L = lib()
    if chunk is None:
        base, per = L.mfvit_boot_work_bytes(n, C, M, 1), 2 * ((n + 7) & ~7)
        chunk = max(16, (WORK_BUDGET - base) // per)
    chunk = max(1, min(int(chunk), R))
    dev = scores.device
    conf = torch.empty(R, M, C, C, device=dev, dtype=torch.int64)
    u2 = torch.empty(R, M, C, device=dev, dtype=torch.int64)
    npos = torch.empty(R, C, device=dev, dtype=torch.int64)
    nbytes = L.mfvit_boot_work_bytes(n, C, M, chunk)
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    ms = scores.stride(0) if M > 1 else 0
    for r0 in range(0, R, chunk):
        k = min(chunk, R - r0)
        check(L.mfvit_boot_counts(scores.data_ptr(), scores.stride(1), ms, labels.data_ptr(), n, C, M, seed, r0, k, int(bool(stratified)),
                                  work.data_ptr(), nbytes, conf[r0].data_ptr(), u2[r0].data_ptr(), npos[r0].data_ptr(), stream()), "mfvit_boot_counts")
    return conf, u2, npos


def delong_counts(scores, labels, want_v2=False):
    """-> (v2 [M, C, n] int32 or None, pos_xy [C, M, M], neg_xy [C, M, M], u2 [M, C], npos [C]) int64 on the GPU (mfvit_delong_counts)"""
    scores, labels, M, n, C = _prepare(scores, labels)
    L = lib()
    dev = scores.device
    v2 = torch.empty(M, C, n, device=dev, dtype=torch.int32) if want_v2 else None
    pos_xy = torch.empty(C, M, M, device=dev, dtype=torch.int64)
    neg_xy = torch.empty(C, M, M, device=dev, dtype=torch.int64)
    u2 = torch.empty(M, C, device=dev, dtype=torch.int64)
    npos = torch.empty(C, device=dev, dtype=torch.int64)
    nbytes = L.mfvit_boot_work_bytes(n, C, M, 1)
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    check(L.mfvit_delong_counts(scores.data_ptr(), scores.stride(1), scores.stride(0) if M > 1 else 0, labels.data_ptr(), n, C, M, work.data_ptr(),
                                nbytes, _lib.ptr(v2), pos_xy.data_ptr(), neg_xy.data_ptr(), u2.data_ptr(), npos.data_ptr(), stream()),
          "mfvit_delong_counts")
    return v2, pos_xy, neg_xy, u2, npos


# ------------------------------------------------------------------------------------------------------------ host arithmetic (float64)
def _ratio(a, b):
    """a / b with 0 / 0 -> 0 (a <= b wherever it is used: b == 0 implies a == 0)"""
    return np.divide(a, b, out=np.zeros_like(a), where=b != 0)


def stats_from_counts(conf, u2, npos, n):
    """int64 arrays conf [R, M, C, C], u2 [R, M, C], npos [R, C] -> dict of float64 arrays: the scalars [R, M], the per-class ones [R, M, C].
    0 / 0 -> 0 for precision / recall / F1; a class without positives or negatives in a replicate has a NaN AUC there, and so has the macro AUC."""
    conf, u2, npos = (np.asarray(a).astype(np.float64) for a in (conf, u2, npos))         # counts < 2^53: exact
    tp = np.diagonal(conf, axis1=2, axis2=3)
    prec, rec = _ratio(tp, conf.sum(2)), _ratio(tp, conf.sum(3))
    f1 = _ratio(2.0 * prec * rec, prec + rec)
    den = 2.0 * npos * (n - npos)
    with np.errstate(invalid="ignore", divide="ignore"):
        auc = np.where(den[:, None, :] > 0, u2 / den[:, None, :], np.nan)
    return {"accuracy": tp.sum(2) / n, "precision": prec, "recall": rec, "f1": f1, "auc": auc, "macro_precision": prec.mean(2),
            "macro_recall": rec.mean(2), "macro_f1": f1.mean(2), "macro_auc": auc.mean(2)}


def percentile_interval(values, level):
    """values [K, ...]: replicates along axis 0 -> (lo, hi, dropped), elementwise over the other axes; NaN replicates are left out and counted"""
    v = np.asarray(values, dtype=np.float64)
    flat = v.reshape(v.shape[0], -1)
    lo, hi = np.full(flat.shape[1], np.nan), np.full(flat.shape[1], np.nan)
    dropped = np.zeros(flat.shape[1], dtype=np.int64)
    a = (1.0 - level) / 2.0
    for j in range(flat.shape[1]):
        keep = flat[~np.isnan(flat[:, j]), j]
        dropped[j] = flat.shape[0] - keep.size
        if keep.size:
            lo[j], hi[j] = np.quantile(keep, [a, 1.0 - a], method="linear")
    shape = v.shape[1:]
    return lo.reshape(shape), hi.reshape(shape), dropped.reshape(shape)


def bootstrap_p_value(delta):
    """delta [K, ...] -> (p, used): two-sided, 2 min((1 + #{d <= 0}) / (K + 1), (1 + #{d >= 0}) / (K + 1)) capped at 1, K the non-NaN replicates"""
    d = np.asarray(delta, dtype=np.float64)
    ok = ~np.isnan(d)
    K = ok.sum(0)
    with np.errstate(invalid="ignore"):
        le, ge = (ok & (d <= 0)).sum(0), (ok & (d >= 0)).sum(0)
    p = np.minimum(1.0, 2.0 * np.minimum((1 + le) / (K + 1.0), (1 + ge) / (K + 1.0)))
    return np.where(K > 0, p, np.nan), K


def _unwrap(x):
    """0-d results as Python numbers"""
    if np.ndim(x):
        return x
    return int(x) if np.issubdtype(np.asarray(x).dtype, np.integer) else float(x)


def summarize(conf, u2, npos, n, level=0.95, names=None):
    """BootstrapResult from the integer arrays of bootstrap_counts (on the host): replicate 0 gives the points, replicates >= 1 the intervals"""
    st = stats_from_counts(conf, u2, npos, n)
    M = st["accuracy"].shape[1]
    names = list(names) if names is not None else [str(m) for m in range(M)]
    if len(names) != M or len(set(names)) != M:
        raise _lib.MfvitError("names must hold one distinct name per score set")
    models, pairs = {}, {}
    for m, nm in enumerate(names):
        models[nm] = {}
        for k, v in st.items():
            lo, hi, dropped = percentile_interval(v[1:, m], level)
            models[nm][k] = Interval(_unwrap(v[0, m]), _unwrap(lo), _unwrap(hi), _unwrap(dropped))
    for a, na in enumerate(names):
        for b, nb in enumerate(names):
            if a == b:
                continue
            pairs[(na, nb)] = {}
            for k, v in st.items():
                d = v[:, a] - v[:, b]
                lo, hi, _ = percentile_interval(d[1:], level)
                p, used = bootstrap_p_value(d[1:])
                pairs[(na, nb)][k] = PairInterval(_unwrap(d[0]), _unwrap(lo), _unwrap(hi), _unwrap(p), _unwrap(used))
    return BootstrapResult(names, level, conf.shape[0] - 1, models, pairs)


def bootstrap_ci(scores, labels, n_boot=2000, level=0.95, seed=0, stratified=False, names=None):
    """Percentile intervals (numpy 'linear' quantiles over the replicates r >= 1) and points (r = 0) of accuracy, per-class and macro precision /
    recall / F1 / AUC for every score set, and for every ordered pair (a, b) the interval of a - b on the same replicates with a two-sided p-value."""
    if not 0.0 < level < 1.0 or n_boot < 1:
        raise _lib.MfvitError("bootstrap_ci wants 0 < level < 1 and n_boot >= 1")
    conf, u2, npos = bootstrap_counts(scores, labels, n_boot, seed, stratified)
    n = labels.shape[0]
    host = torch.cat([conf.view(-1), u2.view(-1), npos.view(-1)]).cpu().numpy()            # one copy
    a, b = conf.numel(), conf.numel() + u2.numel()
    return summarize(host[:a].reshape(conf.shape), host[a:b].reshape(u2.shape), host[b:].reshape(npos.shape), n, level, names)


def delong_from_counts(pos_xy, neg_xy, u2, npos, n, level=0.95, names=None):
    """DeLong, DeLong & Clarke-Pearson (1988) from the exact moments.  With P = npos, N = n - P:
    S10[m][m'] = (P pos_xy - u2_m u2_m') / (4 N^2 P (P - 1)), S01 the same with neg_xy and P, N swapped, Cov = S10 / P + S01 / N.  The numerators
    are formed in Python integers: nothing cancels in floating point.  P < 2 or N < 2: NaN."""
    pos_xy, neg_xy, u2, npos = (np.asarray(a).tolist() for a in (pos_xy, neg_xy, u2, npos))
    M, C = len(u2), len(npos)
    zq = NormalDist().inv_cdf(0.5 + level / 2.0)
    auc, var = np.full((M, C), np.nan), np.full((M, C), np.nan)
    cov, z, p = np.full((C, M, M), np.nan), np.full((C, M, M), np.nan), np.full((C, M, M), np.nan)
    for c in range(C):
        P = npos[c]
        N = n - P
        if P and N:
            for m in range(M):
                auc[m, c] = u2[m][c] / (2 * P * N)
        if P < 2 or N < 2:
            continue
        d10, d01 = 4 * N * N * P * P * (P - 1), 4 * P * P * N * N * (N - 1)
        for a in range(M):
            for b in range(M):
                n10 = P * pos_xy[c][a][b] - u2[a][c] * u2[b][c]
                n01 = N * neg_xy[c][a][b] - u2[a][c] * u2[b][c]
                cov[c, a, b] = (n10 * d01 + n01 * d10) / (d10 * d01)               # integers until this one division
        for m in range(M):
            var[m, c] = cov[c, m, m]
        for a in range(M):
            for b in range(M):
                vd = cov[c, a, a] + cov[c, b, b] - 2.0 * cov[c, a, b]
                if a != b and vd > 0:
                    z[c, a, b] = (auc[a, c] - auc[b, c]) / math.sqrt(vd)
                    p[c, a, b] = math.erfc(abs(z[c, a, b]) / math.sqrt(2.0))
    half = zq * np.sqrt(var)
    names = list(names) if names is not None else [str(m) for m in range(M)]
    return DelongResult(names, level, auc, var, auc - half, auc + half, cov, z, p, np.array(npos, dtype=np.int64), n)


def delong(scores, labels, level=0.95, names=None):
    """Per class: the AUC of every score set with its DeLong variance and normal interval, the covariance matrix between the score sets, and for
    each pair z and p = erfc(|z| / sqrt 2) (NaN where the difference has no variance: a score set against itself or a copy of it)."""
    if not 0.0 < level < 1.0:
        raise _lib.MfvitError("delong wants 0 < level < 1")
    _, pos_xy, neg_xy, u2, npos = delong_counts(scores, labels)
    host = torch.cat([pos_xy.view(-1), neg_xy.view(-1), u2.view(-1), npos.view(-1)]).cpu().numpy()       # one copy
    C, M = pos_xy.shape[0], pos_xy.shape[1]
    k = C * M * M
    return delong_from_counts(host[:k].reshape(C, M, M), host[k:2 * k].reshape(C, M, M), host[2 * k:2 * k + M * C].reshape(M, C), host[2 * k + M * C:],
                              labels.shape[0], level, names)


# --------------------------------------------------------------------------------------- curves, operating points, calibration (device calls)
CurveCounts = namedtuple("CurveCounts", "thr tp fp nthr nnan npos n")
RocCurve = namedtuple("RocCurve", "fpr tpr thresholds")
PrCurve = namedtuple("PrCurve", "precision recall thresholds")
OperatingPoints = namedtuple("OperatingPoints", "names level n_boot at models pairs")
RocBand = namedtuple("RocBand", "names level n_boot fpr tpr lo hi dropped")
Calibration = namedtuple("Calibration", "temperature ece mce brier nll bin_count bin_accuracy bin_confidence used skipped")
MAX_Q, MAX_KT, MAX_NB = 64, 16, 64
POINT_STATS = ("sensitivity", "specificity", "ppv", "npv")


def _i32(t):
    """any 4- or 8-byte tensor as a flat int32 view (what one host copy is made of)"""
    return t.reshape(-1).view(torch.int32)


def curve_counts(scores, labels):
    """scores f32 [n, C] or [M, n, C], labels int64 [n] on the GPU -> CurveCounts on the GPU: thr f32 [M, C, n], tp, fp int32 [M, C, n] (the device
    writes uint32 <= n), nthr, nnan int32 [M, C], npos int64 [C] (include/mfvit.h, mfvit_curve_counts)"""
    scores, labels, M, n, C = _prepare(scores, labels)
    L = lib()
    dev = scores.device
    thr = torch.empty(M, C, n, device=dev, dtype=torch.float32)
    tp = torch.empty(M, C, n, device=dev, dtype=torch.int32)
    fp = torch.empty(M, C, n, device=dev, dtype=torch.int32)
    nthr = torch.empty(M, C, device=dev, dtype=torch.int32)
    nnan = torch.empty(M, C, device=dev, dtype=torch.int32)
    npos = torch.empty(C, device=dev, dtype=torch.int64)
    nbytes = L.mfvit_boot_work_bytes(n, C, M, 1)
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    check(L.mfvit_curve_counts(scores.data_ptr(), scores.stride(1), scores.stride(0) if M > 1 else 0, labels.data_ptr(), n, C, M, work.data_ptr(),
                               nbytes, thr.data_ptr(), tp.data_ptr(), fp.data_ptr(), nthr.data_ptr(), nnan.data_ptr(), npos.data_ptr(), stream()),
          "mfvit_curve_counts")
    return CurveCounts(thr, tp, fp, nthr, nnan, npos, n)


def curve_counts_host(scores, labels):
    """curve_counts as numpy arrays (thr float32, the counts int64) after ONE device-to-host copy"""
    cc = curve_counts(scores, labels)
    M, C, n = cc.thr.shape
    host = torch.cat([_i32(cc.thr), _i32(cc.tp), _i32(cc.fp), _i32(cc.nthr), _i32(cc.nnan), _i32(cc.npos)]).cpu().numpy()
    k, K = M * C * n, M * C
    return CurveCounts(host[:k].view(np.float32).reshape(M, C, n), host[k:2 * k].astype(np.int64).reshape(M, C, n),
                       host[2 * k:3 * k].astype(np.int64).reshape(M, C, n), host[3 * k:3 * k + K].astype(np.int64).reshape(M, C),
                       host[3 * k + K:3 * k + 2 * K].astype(np.int64).reshape(M, C), host[3 * k + 2 * K:].view(np.int64).copy(), n)


def encode_requests(at):
    """[("specificity", x) | ("sensitivity", x) | ("threshold", tau)] -> int32 [Q, 3] rows (kind, a, b) of mfvit_boot_points.  x becomes the exact
    rational Fraction(str(x)).limit_denominator(2**20) = p / q: specificity >= p / q is FP <= floor((q - p) N / q) (kind 0), sensitivity >= p / q is
    TP >= ceil(p P / q) (kind 1); a threshold travels as the bits of its float32 value (kind 2)."""
    from fractions import Fraction
    rows = []
    for what, x in at:
        if what in ("specificity", "sensitivity"):
            f = Fraction(str(x)).limit_denominator(2 ** 20)
            if not 0 <= f <= 1:
                raise _lib.MfvitError(f"{what} must lie in [0, 1], got {x}")
            p, q = f.numerator, f.denominator
            rows.append((0, q - p, q) if what == "specificity" else (1, p, q))
        elif what == "threshold":
            rows.append((2, int(np.array([x], dtype=np.float32).view(np.int32)[0]), 0))
        else:
            raise _lib.MfvitError(f"unknown operating point {what!r}: specificity, sensitivity or threshold")
    if not 1 <= len(rows) <= MAX_Q:
        raise _lib.MfvitError(f"1 .. {MAX_Q} operating points per call")
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


def bootstrap_points(scores, labels, requests, n_boot, seed=0, stratified=False, chunk=None):
    """requests int32 [Q, 3] (encode_requests) -> (tp, fp int32 [n_boot + 1, M, C, Q], thr f32 [n_boot + 1, M, C, Q], npos int64 [n_boot + 1, C]) on
    the GPU; replicate 0 is the sample itself (mfvit_boot_points).  The result does not depend on `chunk`."""
    scores, labels, M, n, C = _prepare(scores, labels)
    if n_boot < 0 or not 0 <= seed < 1 << 64:
        raise _lib.MfvitError("n_boot must be >= 0 and the seed an unsigned 64-bit value")
    req = torch.from_numpy(np.ascontiguousarray(requests, dtype=np.int32).reshape(-1, 3)).to(scores.device)
    Q = req.shape[0]
    if not 1 <= Q <= MAX_Q:
        raise _lib.MfvitError(f"1 .. {MAX_Q} operating points per call")
    R = n_boot + 1
    L = lib()
    if chunk is None:
        base, per = L.mfvit_boot_work_bytes(n, C, M, 1), 2 * ((n + 7) & ~7)
        chunk = max(16, (WORK_BUDGET - base) // per)
    chunk = max(1, min(int(chunk), R))
    dev = scores.device
    tp = torch.empty(R, M, C, Q, device=dev, dtype=torch.int32)
    fp = torch.empty(R, M, C, Q, device=dev, dtype=torch.int32)
    thr = torch.empty(R, M, C, Q, device=dev, dtype=torch.float32)
    npos = torch.empty(R, C, device=dev, dtype=torch.int64)
    nbytes = L.mfvit_boot_work_bytes(n, C, M, chunk)
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    ms = scores.stride(0) if M > 1 else 0
    for r0 in range(0, R, chunk):
        k = min(chunk, R - r0)
        check(L.mfvit_boot_points(scores.data_ptr(), scores.stride(1), ms, labels.data_ptr(), n, C, M, seed, r0, k, int(bool(stratified)), req.data_ptr(), Q,
                                  work.data_ptr(), nbytes, tp[r0].data_ptr(), fp[r0].data_ptr(), thr[r0].data_ptr(), npos[r0].data_ptr(), stream()),
              "mfvit_boot_points")
    return tp, fp, thr, npos


def calib_sums(logits, labels, temps, n_bins=15):
    """logits f32 [n, C] or [M, n, C], labels int64 [n] on the GPU, temps: up to 16 positive floats -> (bin_n, bin_hit int64 [M, Kt, NB], bin_conf f64
    [M, Kt, NB], sums f64 [M, Kt, 3], skipped int64 [M]) on the GPU (mfvit_calib_sums)"""
    import ctypes
    logits, labels, M, n, C = _prepare(logits, labels)
    t32 = np.ascontiguousarray(np.atleast_1d(temps), dtype=np.float32)
    Kt = t32.shape[0]
    if not (1 <= Kt <= MAX_KT and 1 <= n_bins <= MAX_NB and np.isfinite(t32).all() and (t32 > 0).all()):
        raise _lib.MfvitError(f"calibration wants 1 .. {MAX_KT} finite temperatures > 0 and 1 .. {MAX_NB} bins")
    dev = logits.device
    bin_n = torch.empty(M, Kt, n_bins, device=dev, dtype=torch.int64)
    bin_hit = torch.empty(M, Kt, n_bins, device=dev, dtype=torch.int64)
    bin_conf = torch.empty(M, Kt, n_bins, device=dev, dtype=torch.float64)
    sums = torch.empty(M, Kt, 3, device=dev, dtype=torch.float64)
    skipped = torch.empty(M, device=dev, dtype=torch.int64)
    check(lib().mfvit_calib_sums(logits.data_ptr(), logits.stride(1), logits.stride(0) if M > 1 else 0, labels.data_ptr(), n, C, M,
                                 t32.ctypes.data_as(ctypes.c_void_p), Kt, n_bins, bin_n.data_ptr(), bin_hit.data_ptr(), bin_conf.data_ptr(),
                                 sums.data_ptr(), skipped.data_ptr(), stream()), "mfvit_calib_sums")
    return bin_n, bin_hit, bin_conf, sums, skipped


def _calib_host(logits, labels, temps, n_bins):
    """calib_sums as numpy arrays after ONE device-to-host copy"""
    bin_n, bin_hit, bin_conf, sums, skipped = calib_sums(logits, labels, temps, n_bins)
    host = torch.cat([t.reshape(-1).view(torch.int64) for t in (bin_n, bin_hit, bin_conf, sums, skipped)]).cpu().numpy()
    k, s = bin_n.numel(), sums.numel()
    return (host[:k].reshape(bin_n.shape), host[k:2 * k].reshape(bin_n.shape), host[2 * k:3 * k].view(np.float64).reshape(bin_n.shape),
            host[3 * k:3 * k + s].view(np.float64).reshape(sums.shape), host[3 * k + s:].copy())


# ------------------------------------------------------------------------------------------------------------ host arithmetic (float64)
def _column(cc, m, c):
    k = int(cc.nthr[m, c])
    if int(cc.nnan[m, c]) > 0:
        raise ValueError(f"score set {m}, class {c}: {int(cc.nnan[m, c])} NaN scores (scikit-learn refuses NaN input as well)")
    return cc.thr[m, c, :k], cc.tp[m, c, :k].astype(np.float64), cc.fp[m, c, :k].astype(np.float64)


def roc_from_counts(thr, tp, fp, drop_intermediate=True):
    """sklearn.metrics.roc_curve from the arrays of _binary_clf_curve (tp, fp float64, thr float32, highest threshold first): the collinear points
    dropped, the point (0, 0) at threshold inf in front, the rates counts / their last value (NaN arrays when that is 0, as scikit-learn)."""
    if drop_intermediate and len(fp) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fp, 2), np.diff(tp, 2)), True])[0]
        fp, tp, thr = fp[keep], tp[keep], thr[keep]
    tp, fp, thr = np.r_[0.0, tp], np.r_[0.0, fp], np.r_[np.float32(np.inf), thr].astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        fpr = fp / fp[-1] if fp[-1] > 0 else np.full(fp.shape, np.nan)
        tpr = tp / tp[-1] if tp[-1] > 0 else np.full(tp.shape, np.nan)
    return RocCurve(fpr, tpr, thr)


def pr_from_counts(thr, tp, fp, drop_intermediate=False):
    """sklearn.metrics.precision_recall_curve from the same arrays: precision tp / (tp + fp), recall tp / tp[-1] (ones when there is no positive),
    reversed so that recall decreases, closed by the point (precision 1, recall 0)"""
    if drop_intermediate and len(fp) > 2:
        keep = np.where(np.concatenate([[True], np.logical_or(np.diff(tp[:-1]), np.diff(tp[1:])), [True]]))[0]
        fp, tp, thr = fp[keep], tp[keep], thr[keep]
    ps = tp + fp
    precision = np.zeros_like(tp)
    np.divide(tp, ps, out=precision, where=ps != 0)
    recall = np.ones_like(tp) if tp[-1] == 0 else tp / tp[-1]
    return PrCurve(np.hstack((precision[::-1], 1.0)), np.hstack((recall[::-1], 0.0)), thr[::-1])


def ap_from_counts(tp, fp):
    """average precision sum_k (tp_k - tp_{k-1}) / P * tp_k / (tp_k + fp_k) over the thresholds, highest first; NaN without a positive.  The
    increments are differences of integers (exact), so the only roundings are one division and one product per term, the sum and a last division."""
    if len(tp) == 0 or tp[-1] == 0:
        return float("nan")
    ps = tp + fp
    return float(np.sum(np.diff(np.r_[0.0, tp]) * (tp / ps)) / tp[-1])


def _per_column(scores, labels, f):
    cc = curve_counts_host(scores, labels)
    M, C = cc.nthr.shape
    out = [[f(*_column(cc, m, c)) for c in range(C)] for m in range(M)]
    return out if torch.as_tensor(scores).dim() == 3 else out[0]


def roc_curve(scores, labels, drop_intermediate=True):
    """Per class (a list over the classes; for [M, n, C] scores a list of those per score set) RocCurve(fpr, tpr, thresholds) as
    sklearn.metrics.roc_curve(labels == c, scores[:, c]) returns it.  ValueError for a column with NaN scores."""
    return _per_column(scores, labels, lambda thr, tp, fp: roc_from_counts(thr, tp, fp, drop_intermediate))


def precision_recall_curve(scores, labels, drop_intermediate=False):
    """Per class PrCurve(precision, recall, thresholds) as sklearn.metrics.precision_recall_curve"""
    return _per_column(scores, labels, lambda thr, tp, fp: pr_from_counts(thr, tp, fp, drop_intermediate))


def average_precision(scores, labels):
    """Per class sklearn.metrics.average_precision_score, from the same counts: float64 [C] or [M, C]"""
    return np.array(_per_column(scores, labels, lambda thr, tp, fp: ap_from_counts(tp, fp)), dtype=np.float64)


def point_stats(tp, fp, npos, n):
    """int64 arrays tp, fp [R, M, C, Q], npos [R, C] -> dict of float64 [R, M, C, Q]: sensitivity tp / P, specificity (N - fp) / N, ppv tp / (tp + fp),
    npv tn / (tn + fn); NaN where the denominator is 0 (such replicates drop out of an interval and are counted there)"""
    tp, fp = np.asarray(tp).astype(np.float64), np.asarray(fp).astype(np.float64)
    P = np.asarray(npos).astype(np.float64)[:, None, :, None]
    N = n - P
    tn, fn = N - fp, P - tp

    def div(a, b):
        b = np.broadcast_to(b, a.shape)
        return np.divide(a, b, out=np.full(a.shape, np.nan), where=b != 0)
    return {"sensitivity": div(tp, P), "specificity": div(tn, N), "ppv": div(tp, tp + fp), "npv": div(tn, tn + fn)}


def summarize_points(tp, fp, thr, npos, n, at, level=0.95, names=None, stats=POINT_STATS, with_pairs=True):
    """OperatingPoints from the arrays of bootstrap_points (on the host).  models[name][stat] = Interval with [C, Q] arrays (replicate 0 the point,
    replicates >= 1 the percentile interval), models[name]["threshold"] = float32 [C, Q] at replicate 0; pairs[(a, b)]["sensitivity" | "specificity"] =
    PairInterval of a - b on the same replicates with bootstrap_p_value.  `stats` / `with_pairs` leave out what a caller does not read."""
    st = point_stats(tp, fp, npos, n)
    M = tp.shape[1]
    names = list(names) if names is not None else [str(m) for m in range(M)]
    if len(names) != M or len(set(names)) != M:
        raise _lib.MfvitError("names must hold one distinct name per score set")
    models, pairs = {}, {}
    for m, nm in enumerate(names):
        models[nm] = {"threshold": np.asarray(thr)[0, m]}
        for k in stats:
            lo, hi, dropped = percentile_interval(st[k][1:, m], level)
            models[nm][k] = Interval(st[k][0, m], lo, hi, dropped)
    for a, na in enumerate(names):
        for b, nb in enumerate(names):
            if a == b or not with_pairs:
                continue
            pairs[(na, nb)] = {}
            for k in ("sensitivity", "specificity"):
                d = st[k][:, a] - st[k][:, b]
                lo, hi, _ = percentile_interval(d[1:], level)
                p, used = bootstrap_p_value(d[1:])
                pairs[(na, nb)][k] = PairInterval(d[0], lo, hi, p, used)
    return OperatingPoints(names, level, tp.shape[0] - 1, list(at), models, pairs)


def operating_points(scores, labels, at, n_boot=2000, level=0.95, seed=0, stratified=False, names=None):
    """Sensitivity, specificity, PPV and NPV of every score set and class at the operating points `at` - ("specificity", x): the lowest threshold whose
    specificity is at least x; ("sensitivity", x): the highest threshold whose sensitivity is at least x; ("threshold", tau): score >= tau, e.g. a
    threshold locked on the validation set - with bootstrap percentile intervals, and for every ordered pair of score sets the paired difference of
    sensitivity and specificity with its interval and p-value.  In every replicate the threshold is chosen anew for the first two kinds."""
    return _operating_points(scores, labels, at, n_boot, level, seed, stratified, names)


def _operating_points(scores, labels, at, n_boot, level, seed, stratified, names, **what):
    if not 0.0 < level < 1.0 or n_boot < 1:
        raise _lib.MfvitError("operating_points wants 0 < level < 1 and n_boot >= 1")
    at = list(at)
    tp, fp, thr, npos = bootstrap_points(scores, labels, encode_requests(at), n_boot, seed, stratified)
    host = torch.cat([_i32(tp), _i32(fp), _i32(thr), _i32(npos)]).cpu().numpy()                       # one copy
    k = tp.numel()
    return summarize_points(host[:k].astype(np.int64).reshape(tp.shape), host[k:2 * k].astype(np.int64).reshape(tp.shape),
                            host[2 * k:3 * k].view(np.float32).reshape(tp.shape), host[3 * k:].view(np.int64).reshape(npos.shape), labels.shape[0],
                            at, level, names, **what)


def roc_band(scores, labels, grid=None, n_boot=2000, level=0.95, seed=0, stratified=False, names=None):
    """A pointwise confidence band of the ROC curve: operating_points over a grid of specificities (default 21 points 0, 0.05 .. 1; at most 64).
    fpr = 1 - grid [G]; tpr, lo, hi, dropped: dicts name -> [C, G]."""
    grid = [k / 20 for k in range(21)] if grid is None else [float(g) for g in grid]
    op = _operating_points(scores, labels, [("specificity", g) for g in grid], n_boot, level, seed, stratified, names, stats=("sensitivity",),
                           with_pairs=False)
    sens = {nm: op.models[nm]["sensitivity"] for nm in op.names}
    return RocBand(op.names, level, n_boot, 1.0 - np.array(grid), {k: v.point for k, v in sens.items()}, {k: v.lo for k, v in sens.items()},
                   {k: v.hi for k, v in sens.items()}, {k: v.dropped for k, v in sens.items()})


def calibration_from_sums(bin_n, bin_hit, bin_conf, sums, skipped, n, temperature):
    """One (model, temperature): int64 [NB], int64 [NB], float64 [NB], float64 [3], skipped -> Calibration.  ECE = sum_b n_b / N |acc_b - conf_b|, MCE
    the largest gap of a bin that holds a row, N the rows that were not skipped; an empty bin has NaN accuracy and confidence."""
    cnt = np.asarray(bin_n).astype(np.float64)
    used = int(n - int(skipped))
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(cnt > 0, np.asarray(bin_hit) / cnt, np.nan)
        conf = np.where(cnt > 0, np.asarray(bin_conf) / cnt, np.nan)
    gap = np.where(cnt > 0, np.abs(acc - conf), 0.0)
    if used == 0:
        return Calibration(temperature, float("nan"), float("nan"), float("nan"), float("nan"), np.asarray(bin_n), acc, conf, 0, int(skipped))
    return Calibration(temperature, float(np.sum(cnt / used * gap)), float(gap.max()), float(sums[1]) / used, float(sums[0]) / used,
                       np.asarray(bin_n), acc, conf, used, int(skipped))


def calibration(logits, labels, temperature=1.0, n_bins=15):
    """Expected / maximum calibration error, Brier score, NLL and the reliability diagram (per-bin count, accuracy, mean confidence; the bins
    (lo, hi] of Guo et al. 2017) of softmax(logits / temperature).  [n, C] logits -> Calibration; [M, n, C] -> a list, one per score set."""
    temperature = float(np.float32(temperature))
    bin_n, bin_hit, bin_conf, sums, skipped = _calib_host(logits, labels, [temperature], n_bins)
    n = labels.shape[0]
    out = [calibration_from_sums(bin_n[m, 0], bin_hit[m, 0], bin_conf[m, 0], sums[m, 0], skipped[m], n, temperature) for m in range(bin_n.shape[0])]
    return out if logits.dim() == 3 else out[0]


def refine_bracket(slope_at, lo, hi, rel=1e-6, points=MAX_KT, max_rounds=32):
    """The zero of a decreasing function of the temperature (d NLL / d beta: NLL is convex in beta = 1 / T, so its slope changes sign once) inside
    [lo, hi], `points` float32 candidates per round in geometric steps: slope_at(float32 array) -> float64 array, one launch and one host read.  The
    bracket shrinks to the two neighbouring candidates around the sign change until hi - lo <= rel * lo -> (lo, hi).  lo == hi: a candidate with slope
    0, or the end of the first bracket when the sign never changes (slope <= 0 at lo: (lo, lo); slope > 0 at hi: (hi, hi))."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not 0.0 < lo < hi:
        raise _lib.MfvitError("a temperature bracket wants 0 < lo < hi")
    for _ in range(max_rounds):
        t = np.unique(np.float32(lo * (hi / lo) ** (np.arange(points) / (points - 1.0))))
        t[0], t[-1] = np.float32(lo), np.float32(hi)
        t = np.unique(t)
        g = np.asarray(slope_at(t), dtype=np.float64)
        if g[0] <= 0.0:
            return float(t[0]), float(t[0])
        if g[-1] > 0.0:
            return float(t[-1]), float(t[-1])
        k = int(np.argmax(g <= 0.0))                                    # the first candidate at or past the zero; g[k - 1] > 0
        if g[k] == 0.0:
            return float(t[k]), float(t[k])
        new_lo, new_hi = float(t[k - 1]), float(t[k])
        if new_hi - new_lo <= rel * new_lo or (new_lo, new_hi) == (lo, hi):
            return new_lo, new_hi
        lo, hi = new_lo, new_hi
    return lo, hi


def fit_temperature(logits, labels, lo=0.05, hi=20.0):
    """The temperature in [lo, hi] that minimises the NLL of softmax(logits / T) (temperature scaling, Guo et al. 2017): the midpoint of a bracket
    refined below 1e-6 relative (refine_bracket; 16 temperatures per launch, deterministic).  [M, n, C] logits -> one temperature per score set."""
    if logits.dim() == 3:
        return [fit_temperature(logits[m], labels, lo, hi) for m in range(logits.shape[0])]
    a, b = refine_bracket(lambda t: _calib_host(logits, labels, t, 1)[3][0, :, 2], lo, hi)
    return 0.5 * (a + b)


class PairedMeter:
    """Accumulates several score sets over the same samples of an epoch on the device, without a host synchronisation.

        meter = PairedMeter(["sum", "cxr", "enh"], num_classes=3)
        for ...:  meter.update({"sum": out_fus + out_cxr + out_enh, "cxr": out_cxr, "enh": out_enh}, target)
        ci = meter.bootstrap_ci(n_boot=2000);  dl = meter.delong()
    """

    def __init__(self, names, num_classes):
        self.names = list(names)
        if not 1 <= len(self.names) <= MAX_M or len(set(self.names)) != len(self.names):
            raise _lib.MfvitError(f"PairedMeter wants 1 .. {MAX_M} distinct names")
        self.num_classes = num_classes
        self.reset()

    def reset(self):
        self._scores, self._labels = [], []

    def update(self, outputs, target):
        if set(outputs) != set(self.names):
            raise _lib.MfvitError(f"update wants exactly the score sets {self.names}")
        rows = [outputs[k].detach().float() for k in self.names]
        if any(r.dim() != 2 or r.shape != (target.shape[0], self.num_classes) for r in rows):
            raise _lib.MfvitError("every score set must be [batch, num_classes]")
        self._scores.append(torch.stack(rows))
        self._labels.append(target.detach().long().view(-1))

    def gathered(self):
        if not self._scores:
            raise _lib.MfvitError("PairedMeter has seen no batch")
        return torch.cat(self._scores, 1).contiguous(), torch.cat(self._labels, 0).contiguous()

    def bootstrap_ci(self, n_boot=2000, level=0.95, seed=0, stratified=False):
        scores, labels = self.gathered()
        return bootstrap_ci(scores, labels, n_boot, level, seed, stratified, self.names)

    def delong(self, level=0.95):
        scores, labels = self.gathered()
        return delong(scores, labels, level, self.names)

    def operating_points(self, at, n_boot=2000, level=0.95, seed=0, stratified=False):
        scores, labels = self.gathered()
        return operating_points(scores, labels, at, n_boot, level, seed, stratified, self.names)
