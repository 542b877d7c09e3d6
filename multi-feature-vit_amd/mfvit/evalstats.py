"""How certain is an epoch's AUC, and is one score set significantly better than another on the same test set?

The reference's drivers report one number per metric (MAIN_CA:886-911, MAIN_SS:797-821).  This module adds bootstrap percentile intervals,
paired bootstrap tests and DeLong's test for the AUC.  The counting runs on the GPU (csrc/evalstats.hip: every (model, class) column is ordered
once, a replicate then costs O(n) per column); all device results are integers, copied to the host once, and the arithmetic on them is float64
(as EpochMeter.compute does it).

    ci = bootstrap_ci(torch.stack([out_fus + out_cxr + out_enh, out_cxr, out_enh]), target, names=["sum", "cxr", "enh"])
    ci.models["sum"]["macro_auc"]            # Interval(point, lo, hi, dropped)
    ci.pairs[("sum", "cxr")]["macro_auc"]    # PairInterval(point, lo, hi, p, used): delta = sum - cxr
    dl = delong(scores, target)              # dl.auc [M, C], dl.var, dl.lo, dl.hi, dl.cov [C, M, M], dl.z, dl.p
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
