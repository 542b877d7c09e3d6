"""numpy / float64 restatements of the perturbation-test kernels (include/mfvit.h: mfvit_patch_rank, mfvit_patch_perturb,
mfvit_perturb_score).  Test infrastructure only: written from the definitions in the header, not from the kernels."""
import math

import numpy as np


def ref_rank(rel):
    """rank[b][i] = #{j : rel[j] > rel[i], or rel[j] == rel[i] and j < i}, NaN below every number (-inf included), NaNs among themselves by
    index, -0.0 == +0.0 a tie.  rel (B, P) -> int32 (B, P).  The definition, pair by pair (O(P^2) per row, vectorised)."""
    rel = np.asarray(rel, dtype=np.float32)
    B, P = rel.shape
    out = np.empty((B, P), dtype=np.int32)
    idx = np.arange(P)
    for b in range(B):
        r = rel[b]
        nan = np.isnan(r)
        with np.errstate(invalid="ignore"):
            gt = r[None, :] > r[:, None]                             # [i][j]: rel[j] > rel[i]   (False with a NaN on either side)
            eq = r[None, :] == r[:, None]
        gt |= nan[:, None] & ~nan[None, :]                           # every number is above a NaN
        eq |= nan[:, None] & nan[None, :]                            # NaNs tie among themselves
        before = gt | (eq & (idx[None, :] < idx[:, None]))
        out[b] = before.sum(axis=1)
    return out


def inverse_argsort_rank(rel):
    """The inverse permutation of np.argsort(-rel, kind="stable") per row."""
    rel = np.asarray(rel, dtype=np.float32)
    out = np.empty(rel.shape, dtype=np.int32)
    for b in range(rel.shape[0]):
        order = np.argsort(-rel[b], kind="stable")
        out[b, order] = np.arange(rel.shape[1], dtype=np.int32)
    return out


def rank_mismatch(got, ref):
    """The comparison of the GPU test: None when `got` is exactly the reference rank (dtype, shape and every entry), else a message."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != np.int32:
        return f"dtype {got.dtype}, expected int32"
    if got.shape != ref.shape:
        return f"shape {got.shape}, expected {ref.shape}"
    bad = np.argwhere(got != ref)
    if len(bad):
        b, i = bad[0]
        return f"{len(bad)} entries differ, first at image {b} patch {i}: got {got[b, i]}, expected {ref[b, i]}"
    return None


def rank_inputs(kind, B, P, seed):
    """The input classes of the rank tests, f32 (B, P)."""
    g = np.random.Generator(np.random.PCG64(seed))
    if kind == "few_values":
        return g.integers(-2, 3, size=(B, P)).astype(np.float32)
    if kind == "all_equal":
        return np.full((B, P), 0.25, dtype=np.float32)
    if kind == "special":
        pool = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38], dtype=np.float32)
        r = pool[g.integers(0, len(pool), size=(B, P))]
        r.reshape(-1)[:min(len(pool), B * P)] = pool[:min(len(pool), B * P)]      # every special value at least once where it fits
        return r
    if kind == "normal":
        return g.standard_normal((B, P)).astype(np.float32)
    raise ValueError(kind)


RANK_KINDS = ("few_values", "all_equal", "special", "normal")


def ref_perturb(img, rank, ranges, fill):
    """out[s][b][c][y][x] = fill[c] if lo_s <= rank[b][(y // 16) * (W // 16) + x // 16] < hi_s else img[b][c][y][x]."""
    img = np.asarray(img, dtype=np.float32)
    B, C, H, W = img.shape
    gh, gw = H // 16, W // 16
    rank = np.asarray(rank).reshape(B, gh, gw)
    pix = np.repeat(np.repeat(rank, 16, axis=1), 16, axis=2)                  # (B, H, W): the rank of every pixel's patch
    fill = np.asarray(fill, dtype=np.float32).reshape(1, C, 1, 1)
    out = np.empty((len(ranges), B, C, H, W), dtype=np.float32)
    for s, (lo, hi) in enumerate(ranges):
        m = ((pix >= lo) & (pix < hi))[:, None]
        out[s] = np.where(m, fill, img)
    return out


def ref_score(logits, target):
    """(correct [S], nonfinite [S], sums [S][2]) of f32 logits (S, B, C) and targets (B,): float64, exact integer counts; the sums with
    math.fsum (correctly rounded)."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    S, B, C = z.shape
    correct, nonfinite, sums = [0] * S, [0] * S, [[0.0, 0.0] for _ in range(S)]
    for s in range(S):
        probs, logs = [], []
        for b in range(B):
            row, t = z[s, b], int(target[b])
            if not np.isfinite(row).all():
                nonfinite[s] += 1
                continue
            m = row.max()
            e = np.exp(row - m)
            probs.append(float(e[t] / math.fsum(e)))
            logs.append(float(row[t]))
            correct[s] += int(int(np.argmax(row)) == t)                      # np.argmax: the first maximum, as torch.max
        sums[s] = [math.fsum(probs), math.fsum(logs)]
    return correct, nonfinite, sums
