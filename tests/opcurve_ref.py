"""TEST INFRASTRUCTURE ONLY: a numpy restatement of mfvit_curve_counts, mfvit_boot_points and mfvit_calib_sums (include/mfvit.h), written from the
definitions and not from the kernels: every threshold is tried against every sample with a float compare (no ordering, no prefix, no bisection),
in int64 / float64.  The resampling weights and the test cases are evalstats_ref's.  `variant` names a deliberately wrong form (the mutation
checks of test_opcurve_cpu.py)."""
import math

import numpy as np

import evalstats_ref as E


def _candidates(s):
    """the distinct number values of a column, largest first, each as its first holder in index order holds it (-0.0 == +0.0: one value)"""
    ok = ~np.isnan(s)
    vals = np.unique(s[ok] + np.float32(0.0))[::-1]                  # x + 0.0 turns -0.0 into +0.0; np.unique sorts ascending
    first = np.array([int(np.argmax(s == v)) for v in vals], dtype=np.int64)
    return s[first] if vals.size else vals.astype(np.float32)


def _above(s, thr, variant=None):
    """bool [len(thr), n]: sample i is predicted positive at threshold k"""
    with np.errstate(invalid="ignore"):
        m = s[None, :] > thr[:, None] if variant == "gt" else s[None, :] >= thr[:, None]
    if variant == "nan_pred":
        m = m | np.isnan(s)[None, :]
    return m


def curve_counts(scores, labels, variant=None):
    """-> thr f32 [M, C, n] (NaN past nthr), tp, fp int64 [M, C, n] (0 past nthr), nthr, nnan int64 [M, C], npos int64 [C]"""
    scores = np.asarray(scores, dtype=np.float32)
    if scores.ndim == 2:
        scores = scores[None]
    M, n, C = scores.shape
    thr = np.full((M, C, n), np.nan, dtype=np.float32)
    tp, fp = np.zeros((M, C, n), dtype=np.int64), np.zeros((M, C, n), dtype=np.int64)
    nthr, nnan = np.zeros((M, C), dtype=np.int64), np.zeros((M, C), dtype=np.int64)
    npos = np.array([(labels == c).sum() for c in range(C)], dtype=np.int64)
    for m in range(M):
        for c in range(C):
            s = scores[m, :, c]
            pos = (labels == c).astype(np.int64)
            cand = _candidates(s)
            G = cand.size
            nthr[m, c], nnan[m, c] = G, np.isnan(s).sum()
            thr[m, c, :G] = cand
            for k0 in range(0, G, 512):
                k1 = min(k0 + 512, G)
                a = _above(s, cand[k0:k1], variant).astype(np.int64)
                tp[m, c, k0:k1] = a @ pos
                fp[m, c, k0:k1] = a @ (1 - pos)
    return thr, tp, fp, nthr, nnan, npos


def request_rows(at):
    """the (kind, a, b) rows of mfvit_boot_points, from the definitions of mfvit.evalstats.encode_requests"""
    from fractions import Fraction
    rows = []
    for what, x in at:
        if what == "threshold":
            rows.append((2, int(np.array([x], dtype=np.float32).view(np.int32)[0]), 0))
        else:
            f = Fraction(str(x)).limit_denominator(2 ** 20)
            rows.append((0, f.denominator - f.numerator, f.denominator) if what == "specificity" else (1, f.numerator, f.denominator))
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


def boot_points(scores, labels, seed, r0, R, stratified, requests, variant=None):
    """-> tp, fp int64 [R, M, C, Q], thr f32 [R, M, C, Q], npos int64 [R, C]: per replicate a scan over EVERY candidate threshold"""
    scores = np.asarray(scores, dtype=np.float32)
    if scores.ndim == 2:
        scores = scores[None]
    M, n, C = scores.shape
    req = np.asarray(requests).reshape(-1, 3)
    Q = req.shape[0]
    tp, fp = np.zeros((R, M, C, Q), dtype=np.int64), np.zeros((R, M, C, Q), dtype=np.int64)
    thr = np.zeros((R, M, C, Q), dtype=np.float32)
    npos = np.zeros((R, C), dtype=np.int64)
    W = np.stack([E.weights(n, seed, r0 + k, labels, C, stratified) for k in range(R)])          # [R, n]
    inf = np.array([np.inf], dtype=np.float32)
    for c in range(C):
        pos = (labels == c).astype(np.int64)
        npos[:, c] = W @ pos
        for m in range(M):
            s = scores[m, :, c]
            cand = np.concatenate([inf[:1], _candidates(s)])            # highest first; "above everything" in front
            above = _above(s, cand, variant).astype(np.int64)
            above[0] = 0                                                 # (+inf scores are >= inf: the extra threshold still includes nothing)
            TP, FP = (W * pos) @ above.T, (W * (1 - pos)) @ above.T      # [R, G + 1]
            for q, (kind, a, b) in enumerate(req.tolist()):
                if kind == 2:
                    tau = np.array([a], dtype=np.int32).view(np.float32)
                    inc = _above(s, tau, variant)[0]
                    tp[:, m, c, q], fp[:, m, c, q] = W @ (inc * pos), W @ (inc * (1 - pos))
                    with np.errstate(invalid="ignore"):
                        took = cand[1:][cand[1:] >= tau[0]]
                    thr[:, m, c, q] = took[-1] if took.size else np.inf
                    continue
                for r in range(R):
                    P = int(npos[r, c])
                    N = n - P
                    if kind == 0:                                   # the lowest threshold (last candidate) within the cap; candidate 0 always is
                        j = int(np.nonzero(FP[r] <= (a * N) // b)[0].max())
                    else:                                           # the highest threshold (first candidate) that reaches the need, else the lowest
                        need = (a * P) // b if variant == "floor" else -((-a * P) // b)
                        ok = np.nonzero(TP[r] >= need)[0]
                        j = int(ok.min()) if ok.size else cand.size - 1
                    tp[r, m, c, q], fp[r, m, c, q], thr[r, m, c, q] = TP[r, j], FP[r, j], cand[j]
    return tp, fp, thr, npos


def calib_sums(logits, labels, temps, NB, variant=None):
    """-> dict: bin_n, bin_hit int64 [M, Kt, NB], bin_conf f64 [M, Kt, NB], sums f64 [M, Kt, 3], skipped int64 [M], and for the tests' gates
    conf f64 [M, Kt, n] (NaN for a skipped row) and abs_sums f64 [M, Kt, 3] = the sums of the magnitudes of the terms' parts"""
    logits = np.asarray(logits, dtype=np.float32)
    if logits.ndim == 2:
        logits = logits[None]
    M, n, C = logits.shape
    temps = np.atleast_1d(np.asarray(temps, dtype=np.float32))
    Kt = temps.size
    out = dict(bin_n=np.zeros((M, Kt, NB), dtype=np.int64), bin_hit=np.zeros((M, Kt, NB), dtype=np.int64), bin_conf=np.zeros((M, Kt, NB)),
               sums=np.zeros((M, Kt, 3)), skipped=np.zeros(M, dtype=np.int64), conf=np.full((M, Kt, n), np.nan), abs_sums=np.zeros((M, Kt, 3)))
    valid = (labels >= 0) & (labels < C)
    for m in range(M):
        z = logits[m].astype(np.float64)
        use = np.isfinite(logits[m]).all(1) & valid
        out["skipped"][m] = n - use.sum()
        z, y = z[use], labels[use]
        rows = np.arange(z.shape[0])
        top = np.argmax(z, axis=1) if z.size else np.zeros(0, dtype=np.int64)
        d = z - z.max(axis=1, keepdims=True) if z.size else z
        for k in range(Kt):
            beta = 1.0 / np.float64(temps[k])
            e = np.exp(beta * d)
            den = np.cumsum(e, axis=1)[:, -1]                            # c ascending, one add at a time: the order the header states
            p = e / den[:, None]
            conf = p[rows, top]
            if variant == "lo_hi_open":
                b = np.minimum(NB - 1, np.floor(conf * NB).astype(np.int64))
            else:
                b = np.minimum(NB - 1, np.maximum(0, np.ceil(conf * NB).astype(np.int64) - 1))
            out["conf"][m, k, use] = conf
            out["bin_n"][m, k] = np.bincount(b, minlength=NB)
            out["bin_hit"][m, k] = np.bincount(b[top == y], minlength=NB)
            out["bin_conf"][m, k] = [math.fsum(conf[b == j]) for j in range(NB)]
            onehot = np.zeros_like(p)
            onehot[rows, y] = 1.0
            terms = (np.log(den) - beta * d[rows, y], ((p - onehot) ** 2).sum(1), (p * d).sum(1) - d[rows, y])
            out["sums"][m, k] = [math.fsum(t) for t in terms]           # correctly rounded sums: the restatement adds no error of its own order
            # the first two terms are sums of non-negative parts; the third is a difference, whose parts are what an error is relative to
            out["abs_sums"][m, k] = [terms[0].sum(), terms[1].sum(), ((p * np.abs(d)).sum(1) + np.abs(d[rows, y])).sum()]
    return out


def edge_margin(conf, NB):
    """the smallest distance of a confidence to an INNER bin edge k / NB, k = 1 .. NB - 1, over the rows that are not NaN.  (The outer edges
    decide nothing: a confidence is at least 1 / C > 0, and one that rounds to 1.0 or just below it has ceil(conf NB) = NB either way.)"""
    c = conf[~np.isnan(conf)] * NB
    if NB < 2 or not c.size:
        return float("inf")
    return float(np.min(np.abs(c - np.clip(np.round(c), 1, NB - 1))) / NB)


def calibration_direct(logits, labels, T, NB):
    """(ece, mce, brier, nll) of softmax(logits / T) for one score set without skipped rows - torch.softmax in float64, the (lo, hi] bins of Guo et al."""
    import torch
    p = torch.softmax(torch.from_numpy(np.asarray(logits, dtype=np.float32)).double() / float(np.float32(T)), dim=1).numpy()
    n, C = p.shape
    conf, pred = p.max(1), np.argmax(np.asarray(logits), axis=1)
    ece, mce = 0.0, 0.0
    for k in range(NB):
        inb = (conf > k / NB) & (conf <= (k + 1) / NB)
        if inb.any():
            gap = abs((pred[inb] == labels[inb]).mean() - conf[inb].mean())
            ece, mce = ece + inb.sum() / n * gap, max(mce, gap)
    onehot = np.eye(C)[labels]
    return ece, mce, float(((p - onehot) ** 2).sum(1).mean()), float(-np.log(p[np.arange(n), labels]).mean())
