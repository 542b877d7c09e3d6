"""TEST INFRASTRUCTURE ONLY: a numpy restatement of the bootstrap / DeLong definitions of include/mfvit.h (mfvit_boot_counts,
mfvit_delong_counts) and of the host arithmetic of mfvit.evalstats.  Written from the definitions, not from the kernels: the hash in uint64
arithmetic, weights from np.bincount, every (positive, negative) pair compared (O(n^2)), and a second sort-based statement for large n."""
import math
from fractions import Fraction
from statistics import NormalDist

import numpy as np

M32 = 0xFFFFFFFF


def lowbias32(x):
    """x: uint64 array (or int) holding 32-bit values"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x


def replicate_key(seed, r):
    lo, hi = seed & M32, (seed >> 32) & M32
    inner = int(lowbias32((hi + 0x9E3779B9 * (r + 1)) & M32))
    return int(lowbias32(lo ^ inner))


def strata_of(labels, C):
    labels = np.asarray(labels, dtype=np.int64)
    return np.where((labels >= 0) & (labels < C), labels, C)


def weights(n, seed, r, labels=None, C=None, stratified=False, key=None):
    """w_r[i], int64 [n]: how often sample i is drawn in replicate r"""
    if r == 0:
        return np.ones(n, dtype=np.int64)
    key = replicate_key(seed, r) if key is None else key
    h = lowbias32(np.arange(n, dtype=np.uint64) ^ np.uint64(key))
    if not stratified:
        idx = (h * np.uint64(n)) >> np.uint64(32)
        return np.bincount(idx.astype(np.int64), minlength=n).astype(np.int64)
    s = strata_of(labels, C)
    L = np.argsort(s, kind="stable")
    ss = s[L]
    off = np.searchsorted(ss, ss, side="left").astype(np.uint64)
    ns = (np.searchsorted(ss, ss, side="right") - off.astype(np.int64)).astype(np.uint64)
    idx = L[(off + ((h * ns) >> np.uint64(32))).astype(np.int64)]
    return np.bincount(idx, minlength=n).astype(np.int64)


def preds_of(scores):
    """[M, n, C] -> [M, n]: the first maximum, the first NaN before it (np.argmax, torch.max)"""
    return np.argmax(scores, axis=-1)


def conf_weighted(scores, labels, w):
    M, n, C = scores.shape
    out = np.zeros((M, C, C), dtype=np.int64)
    pr = preds_of(scores)
    for m in range(M):
        for i in range(n):
            t = int(labels[i])
            if 0 <= t < C:
                out[m, t, pr[m, i]] += int(w[i])
    return out


def psi2(a, b):
    """2 [a > b] + [a == b] on float32 arrays, broadcast; NaN compares false both ways"""
    with np.errstate(invalid="ignore"):
        return 2 * (a > b).astype(np.int64) + (a == b).astype(np.int64)


def u2_brute(scores, labels, w, variant=None):
    """u2 [M, C], npos [C] by the definition: every pair.  `variant` names a deliberately wrong form (the mutation checks)."""
    M, n, C = scores.shape
    u2 = np.zeros((M, C), dtype=np.int64)
    npos = np.zeros(C, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    for c in range(C):
        pos, neg = labels == c, labels != c
        npos[c] = w[pos].sum()
        for m in range(M):
            s = scores[m, :, c]
            if variant == "nan_smallest":
                s = np.where(np.isnan(s), -np.inf, s)
            k = psi2(s[pos][:, None], s[neg][None, :])
            if variant == "no_tie_credit":
                k = k - (k == 1)
            wi = w[pos][:, None]
            wj = np.ones_like(w[neg])[None, :] if variant == "one_sided" else w[neg][None, :]
            u2[m, c] = int((wi * wj * k).sum())
    return u2, npos


def u2_sorted(scores, labels, w):
    """The same numbers from a sort and two searches per column (for large n).  NaN scores are left out of every pair; they stay in npos."""
    M, n, C = scores.shape
    u2 = np.zeros((M, C), dtype=np.int64)
    npos = np.zeros(C, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    for c in range(C):
        npos[c] = w[labels == c].sum()
        for m in range(M):
            s = scores[m, :, c]
            ok = ~np.isnan(s)
            pos, neg = ok & (labels == c), ok & (labels != c)
            order = np.argsort(s[neg], kind="stable")
            sn = s[neg][order]
            cw = np.concatenate([[0], np.cumsum(w[neg][order])])
            lt = np.searchsorted(sn, s[pos], side="left")
            le = np.searchsorted(sn, s[pos], side="right")
            u2[m, c] = int((w[pos] * (cw[lt] + cw[le])).sum())
    return u2, npos


def boot_counts(scores, labels, seed, r0, R, stratified=False, brute=True, key_of=None):
    """(conf [R, M, C, C], u2 [R, M, C], npos [R, C]) int64 for replicates r0 .. r0 + R - 1"""
    scores = np.asarray(scores, dtype=np.float32)
    if scores.ndim == 2:
        scores = scores[None]
    M, n, C = scores.shape
    conf = np.zeros((R, M, C, C), dtype=np.int64)
    u2 = np.zeros((R, M, C), dtype=np.int64)
    npos = np.zeros((R, C), dtype=np.int64)
    for k in range(R):
        r = r0 + k
        w = weights(n, seed, r, labels, C, stratified, key=None if key_of is None else key_of(seed, r))
        conf[k] = conf_weighted(scores, labels, w)
        u2[k], npos[k] = (u2_brute if brute else u2_sorted)(scores, labels, w)
    return conf, u2, npos


def v2_brute(scores, labels):
    """int64 [M, C, n]"""
    M, n, C = scores.shape
    v2 = np.zeros((M, C, n), dtype=np.int64)
    for m in range(M):
        for c in range(C):
            s = scores[m, :, c]
            pos, neg = labels == c, labels != c
            k = psi2(s[pos][:, None], s[neg][None, :])             # [P, N]
            v2[m, c, pos] = k.sum(1)
            v2[m, c, neg] = k.sum(0)
    return v2


def v2_sorted(scores, labels):
    M, n, C = scores.shape
    v2 = np.zeros((M, C, n), dtype=np.int64)
    for m in range(M):
        for c in range(C):
            s = scores[m, :, c]
            ok = ~np.isnan(s)
            pos, neg = ok & (labels == c), ok & (labels != c)
            sn, sp = np.sort(s[neg]), np.sort(s[pos])
            v2[m, c, pos] = np.searchsorted(sn, s[pos], side="left") + np.searchsorted(sn, s[pos], side="right")
            v2[m, c, neg] = 2 * sp.size - np.searchsorted(sp, s[neg], side="left") - np.searchsorted(sp, s[neg], side="right")
    return v2


def delong_counts(scores, labels, brute=True):
    """(v2 [M, C, n], pos_xy [C, M, M], neg_xy [C, M, M], u2 [M, C], npos [C]) int64"""
    scores = np.asarray(scores, dtype=np.float32)
    if scores.ndim == 2:
        scores = scores[None]
    M, n, C = scores.shape
    v2 = (v2_brute if brute else v2_sorted)(scores, labels)
    pos_xy = np.zeros((C, M, M), dtype=np.int64)
    neg_xy = np.zeros((C, M, M), dtype=np.int64)
    u2 = np.zeros((M, C), dtype=np.int64)
    npos = np.zeros(C, dtype=np.int64)
    for c in range(C):
        pos = labels == c
        npos[c] = pos.sum()
        for a in range(M):
            u2[a, c] = v2[a, c, pos].sum()
            for b in range(M):
                pos_xy[c, a, b] = int((v2[a, c, pos] * v2[b, c, pos]).sum())
                neg_xy[c, a, b] = int((v2[a, c, ~pos] * v2[b, c, ~pos]).sum())
    return v2, pos_xy, neg_xy, u2, npos


# ------------------------------------------------------------------------------------------------------------ host formulas
def _div0(a, b):
    return a / b if b else 0.0


def stats_of(conf, u2, npos, n):
    """One replicate, one model: conf [C, C], u2 [C], npos [C] -> dict of floats / lists"""
    C = len(npos)
    out = {"accuracy": sum(int(conf[c][c]) for c in range(C)) / n}
    prec, rec, f1, auc = [], [], [], []
    for c in range(C):
        tp = int(conf[c][c])
        col = sum(int(conf[t][c]) for t in range(C))
        row = sum(int(conf[c][p]) for p in range(C))
        p, r = _div0(tp, col), _div0(tp, row)
        prec.append(p), rec.append(r), f1.append(_div0(2 * p * r, p + r))
        P = int(npos[c])
        auc.append(int(u2[c]) / (2.0 * P * (n - P)) if P and n - P else float("nan"))
    out.update(precision=prec, recall=rec, f1=f1, auc=auc, macro_precision=sum(prec) / C, macro_recall=sum(rec) / C, macro_f1=sum(f1) / C,
               macro_auc=sum(auc) / C)
    return out


def interval(values, level):
    """percentile interval (numpy 'linear') of the non-NaN values: (lo, hi, number left out)"""
    v = np.asarray(values, dtype=np.float64)
    keep = v[~np.isnan(v)]
    if keep.size == 0:
        return float("nan"), float("nan"), int(v.size)
    a = (1.0 - level) / 2.0
    lo, hi = np.quantile(keep, [a, 1.0 - a], method="linear")
    return float(lo), float(hi), int(v.size - keep.size)


def p_two_sided(delta):
    d = np.asarray(delta, dtype=np.float64)
    d = d[~np.isnan(d)]
    K = d.size
    if K == 0:
        return float("nan"), 0
    return min(1.0, 2.0 * min((1 + int((d <= 0).sum())) / (K + 1), (1 + int((d >= 0).sum())) / (K + 1))), K


def bootstrap_ci_ref(scores, labels, n_boot, level, seed, stratified=False):
    """(models, pairs): models[m][stat] = (point, lo, hi, dropped) and pairs[(a, b)][stat] = (point, lo, hi, p, used), every entry a flat list over
    the classes (one element for a scalar statistic) - the definitions of mfvit.evalstats.bootstrap_ci, one replicate and one element at a time"""
    scores = np.asarray(scores, dtype=np.float32)
    if scores.ndim == 2:
        scores = scores[None]
    M, n, C = scores.shape
    conf, u2, npos = boot_counts(scores, labels, seed, 0, n_boot + 1, stratified, brute=False)
    per = [[stats_of(conf[r, m], u2[r, m], npos[r], n) for m in range(M)] for r in range(n_boot + 1)]
    col = lambda m, k: np.array([per[r][m][k] for r in range(n_boot + 1)], dtype=np.float64).reshape(n_boot + 1, -1)
    models, pairs = {}, {}
    for m in range(M):
        models[m] = {}
        for k in per[0][0]:
            v = col(m, k)
            iv = [interval(v[1:, j], level) for j in range(v.shape[1])]
            models[m][k] = (v[0].tolist(), [x[0] for x in iv], [x[1] for x in iv], [x[2] for x in iv])
    for a in range(M):
        for b in range(M):
            if a == b:
                continue
            pairs[(a, b)] = {}
            for k in per[0][0]:
                d = col(a, k) - col(b, k)
                iv = [interval(d[1:, j], level) for j in range(d.shape[1])]
                pv = [p_two_sided(d[1:, j]) for j in range(d.shape[1])]
                pairs[(a, b)][k] = (d[0].tolist(), [x[0] for x in iv], [x[1] for x in iv], [x[0] for x in pv], [x[1] for x in pv])
    return models, pairs


def delong_from_counts(pos_xy, neg_xy, u2, npos, n, level=0.95):
    """dict of arrays: auc [M, C], var [M, C], lo, hi [M, C], cov [C, M, M], z [C, M, M], p [C, M, M]; exact rationals first"""
    C, M = len(npos), len(u2)
    zq = NormalDist().inv_cdf(0.5 + level / 2.0)
    nan = float("nan")
    out = dict(auc=np.full((M, C), nan), var=np.full((M, C), nan), lo=np.full((M, C), nan), hi=np.full((M, C), nan), cov=np.full((C, M, M), nan),
               z=np.full((C, M, M), nan), p=np.full((C, M, M), nan))
    for c in range(C):
        P = int(npos[c])
        N = n - P
        if P and N:
            for m in range(M):
                out["auc"][m, c] = int(u2[m][c]) / (2.0 * P * N)
        if P < 2 or N < 2:
            continue
        for a in range(M):
            for b in range(M):
                ua, ub = int(u2[a][c]), int(u2[b][c])
                s10 = Fraction(P * int(pos_xy[c][a][b]) - ua * ub, 4 * N * N * P * (P - 1))
                s01 = Fraction(N * int(neg_xy[c][a][b]) - ua * ub, 4 * P * P * N * (N - 1))
                out["cov"][c, a, b] = float(s10 / P + s01 / N)
        for m in range(M):
            v = out["cov"][c, m, m]
            out["var"][m, c] = v
            out["lo"][m, c] = out["auc"][m, c] - zq * math.sqrt(v)
            out["hi"][m, c] = out["auc"][m, c] + zq * math.sqrt(v)
        for a in range(M):
            for b in range(M):
                vd = out["cov"][c, a, a] + out["cov"][c, b, b] - 2.0 * out["cov"][c, a, b]
                if a != b and vd > 0:
                    z = (out["auc"][a, c] - out["auc"][b, c]) / math.sqrt(vd)
                    out["z"][c, a, b] = z
                    out["p"][c, a, b] = math.erfc(abs(z) / math.sqrt(2.0))
    return out


def delong_direct(scores, labels, c):
    """The psi-matrix definition in float64 for one class: (auc [M], cov [M, M]) - DeLong, DeLong & Clarke-Pearson 1988, eqs. 3-6"""
    scores = np.asarray(scores, dtype=np.float32)
    M = scores.shape[0]
    pos, neg = labels == c, labels != c
    P, N = int(pos.sum()), int(neg.sum())
    v10, v01, theta = [], [], []
    for m in range(M):
        s = scores[m, :, c]
        psi = psi2(s[pos][:, None], s[neg][None, :]).astype(np.float64) / 2.0
        v10.append(psi.mean(1)), v01.append(psi.mean(0)), theta.append(psi.mean())
    v10, v01 = np.array(v10), np.array(v01)
    s10 = np.cov(v10, ddof=1).reshape(M, M)
    s01 = np.cov(v01, ddof=1).reshape(M, M)
    return np.array(theta), s10 / P + s01 / N


# ------------------------------------------------------------------------------------------------------------ cases
def case(n, C, M, kind, lkind, seed):
    """scores f32 [M, n, C], labels int64 [n].  kind: gauss | ties (quantised to 1/8) | equal | special (NaN, +-inf, +-0 sprinkled in);
    lkind: random | outside (a third outside [0, C)) | missing (the last class has no sample)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s = rng.standard_normal((M, n, C)).astype(np.float32)
    if kind == "ties":
        s = (np.round(s * 8) / 8).astype(np.float32)
    elif kind == "equal":
        s[:] = 0.25
    elif kind == "special":
        s = (np.round(s * 4) / 4).astype(np.float32)
        u = rng.random((M, n, C))
        s[u < 0.08] = np.nan
        s[(u >= 0.08) & (u < 0.14)] = np.inf
        s[(u >= 0.14) & (u < 0.20)] = -np.inf
        s[(u >= 0.20) & (u < 0.28)] = 0.0
        s[(u >= 0.28) & (u < 0.36)] = -0.0
    p = np.arange(C, 0, -1, dtype=np.float64)
    t = rng.choice(C, size=n, p=p / p.sum()).astype(np.int64)
    if lkind == "missing":
        t[t == C - 1] = C - 2 if C > 1 else -1
    elif lkind == "outside":
        pick = rng.random(n) < 1 / 3
        t[pick] = np.array([-1, C, 2 ** 32 + 1], dtype=np.int64)[np.arange(n) % 3][pick]
    return np.ascontiguousarray(s), t
