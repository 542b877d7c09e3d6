"""Float64 numpy reference for the CKA kernels (csrc/cka.hip, mfvit/similarity.py) and the gates the tests hold them to.

Definitions (include/mfvit.h): the centred Gram K = Xc Xc' (Xc = X minus each column's mean over the n rows), the unbiased HSIC estimator of
Song et al. 2012 (HSIC1) and the biased one (HSIC0 = tr(K H L H) / (n - 1)^2), minibatch CKA of Nguyen, Raghu & Kornblith 2021.  HSIC1 is
written a second time as the brute-force U-statistic over distinct index tuples and biased CKA a second time in feature space
(Kornblith et al. 2019, eq. 4), so that the formulas the kernels are checked against are themselves pinned (tests/test_cka_cpu.py).

The gates are derived from the arithmetic, as tests/wgrad_ref.py derives its own:
  * Gram.  The kernel multiplies f32 values centred by ITS f32 column mean; the reference centres in double.  Both estimators, and the
    double-centred matrix H g H, do not depend on the shift, so device and reference are compared after double centring on the host.  Every one
    of the k products of an element enters one f32 add (relative 2^-24 each, at most k of them ahead of it in the chain), each centred operand
    carries one rounding of its own (2 more), and the splits' partials are added in double (nothing at this scale); one more unit covers the
    conversion.  Hence  E_ij = (k + 3) 2^-24 sum_c |xc_ic| |xc_jc|, and through H . H:  E_ij + rowmean(E)_i + colmean(E)_j + mean(E).
  * HSIC.  Each of the three sums (sum K o L, (1'K1)(1'L1), sum_a rowsum(K)_a rowsum(L)_a) has at most n^2 terms added in double in some
    order: within 4 n^2 2^-53 of the sum of its absolute terms; the gate of an HSIC value is those three bounds through the estimator's own
    coefficients.
"""
import itertools

import numpy as np

U24 = 2.0 ** -24
U53 = 2.0 ** -53


def centered(x):
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    return x - x.mean(axis=0, keepdims=True)


def gram_centered(x):
    xc = centered(x)
    return xc @ xc.T


def double_center(g):
    g = np.asarray(g, dtype=np.float64)
    return g - g.mean(axis=0, keepdims=True) - g.mean(axis=1, keepdims=True) + g.mean()


def gram_gate(x):
    """Elementwise bound on | H g_device H - H K H | for the f32 kernel (module docstring)."""
    xc = np.abs(centered(x))
    k = xc.shape[1]
    e = (k + 3) * U24 * (xc @ xc.T)
    return e + e.mean(axis=1, keepdims=True) + e.mean(axis=0, keepdims=True) + e.mean()


def _sums(K, L, unbiased):
    K, L = np.array(K, dtype=np.float64), np.array(L, dtype=np.float64)
    if unbiased:
        np.fill_diagonal(K, 0.0)
        np.fill_diagonal(L, 0.0)
    return (K * L).sum(), K.sum() * L.sum(), (K.sum(axis=1) * L.sum(axis=1)).sum()


def _coef(n, unbiased):
    """HSIC = (s1 + c2 s2 - c3 s3) / den from the three sums."""
    n = float(n)
    if unbiased:
        return 1.0 / ((n - 1) * (n - 2)), 2.0 / (n - 2), n * (n - 3)
    return 1.0 / (n * n), 2.0 / n, (n - 1) ** 2


def hsic(K, L, unbiased=True):
    n = len(K)
    s1, s2, s3 = _sums(K, L, unbiased)
    c2, c3, den = _coef(n, unbiased)
    return (s1 + c2 * s2 - c3 * s3) / den


def hsic1(K, L):
    return hsic(K, L, True)


def hsic0(K, L):
    return hsic(K, L, False)


def hsic0_trace(K, L):
    """tr(K H L H) / (n - 1)^2, literally."""
    n = len(K)
    H = np.eye(n) - 1.0 / n
    return np.trace(K @ H @ L @ H) / (n - 1) ** 2


def hsic_gate(K, L, unbiased=True):
    n = len(K)
    a1, a2, a3 = _sums(np.abs(K), np.abs(L), unbiased)
    c2, c3, den = _coef(n, unbiased)
    return 4.0 * n * n * U53 * (a1 + c2 * a2 + c3 * a3) / abs(den)


def hsic1_ustat(K, L):
    """The U-statistic over distinct index tuples (Song et al. 2012, eq. 4 expanded):
    sum_{i != j} K_ij L_ij / (n)_2 + sum_{i,j,q,r distinct} K_ij L_qr / (n)_4 - 2 sum_{i,j,q distinct} K_ij L_iq / (n)_3."""
    K, L = np.asarray(K, dtype=np.float64), np.asarray(L, dtype=np.float64)
    n = len(K)
    t2 = sum(K[i, j] * L[i, j] for i, j in itertools.permutations(range(n), 2))
    t4 = sum(K[i, j] * L[q, r] for i, j, q, r in itertools.permutations(range(n), 4))
    t3 = sum(K[i, j] * L[i, q] for i, j, q in itertools.permutations(range(n), 3))
    return t2 / (n * (n - 1)) + t4 / (n * (n - 1) * (n - 2) * (n - 3)) - 2.0 * t3 / (n * (n - 1) * (n - 2))


def cka_from_grams(Ks, Ls, unbiased=True):
    """Minibatch CKA from lists of Gram matrices (one per minibatch)."""
    ab = sum(hsic(K, L, unbiased) for K, L in zip(Ks, Ls))
    aa = sum(hsic(K, K, unbiased) for K in Ks)
    bb = sum(hsic(L, L, unbiased) for L in Ls)
    with np.errstate(invalid="ignore", divide="ignore"):      # (a constant representation: 0 / 0, NaN)
        return ab / np.sqrt(aa * bb)


def cka(x, y, unbiased=True):
    return cka_from_grams([gram_centered(x)], [gram_centered(y)], unbiased)


def cka_feature_space(x, y):
    """Biased linear CKA in feature space: ||Yc'Xc||_F^2 / (||Xc'Xc||_F ||Yc'Yc||_F)."""
    xc, yc = centered(x), centered(y)
    return np.linalg.norm(yc.T @ xc) ** 2 / (np.linalg.norm(xc.T @ xc) * np.linalg.norm(yc.T @ yc))


def cka_matrix(stacks_a, stacks_b, unbiased=True):
    """(Ra, Rb) minibatch CKA: stacks_a / stacks_b are lists (one entry per minibatch) of (R, n, ...) arrays."""
    Ka = [[gram_centered(r) for r in s] for s in stacks_a]
    Kb = [[gram_centered(r) for r in s] for s in stacks_b]
    ra, rb = len(Ka[0]), len(Kb[0])
    out = np.empty((ra, rb))
    for i in range(ra):
        for j in range(rb):
            out[i, j] = cka_from_grams([k[i] for k in Ka], [k[j] for k in Kb], unbiased)
    return out


def gram_f32_emulated(x, n_chunks=7):
    """An honest f32 Gram in an order no kernel uses: f32 column means summed from the last row up, one f32 rounding per centred operand, each
    element's products added in f32 from the LAST column to the first inside n_chunks interleaved column classes, the classes added in
    double."""
    x = np.asarray(x, dtype=np.float32).reshape(len(x), -1)
    n, k = x.shape
    s = np.zeros(k, dtype=np.float32)
    for row in range(n - 1, -1, -1):
        s = (s + x[row]).astype(np.float32)
    m = (s / np.float32(n)).astype(np.float32)
    xc = (x - m).astype(np.float32)
    g = np.zeros((n, n), dtype=np.float64)
    for c in range(n_chunks):
        acc = np.zeros((n, n), dtype=np.float32)
        for col in range(k - 1 - c, -1, -n_chunks):
            acc = (acc + np.outer(xc[:, col], xc[:, col]).astype(np.float32)).astype(np.float32)
        g += acc.astype(np.float64)
    return g


def exact_inputs(n, k, seed):
    """Integers in [-4, 4], the rows in +- pairs plus a zero row for odd n: every column mean is exactly 0 and every sum is exact in f32."""
    g = np.random.Generator(np.random.PCG64(seed))
    half = g.integers(-4, 5, size=(n // 2, k))
    rows = [half, -half] + ([np.zeros((1, k), dtype=half.dtype)] if n % 2 else [])
    x = np.concatenate(rows, axis=0)
    return x[g.permutation(n)].astype(np.int64)


def offset_gaussians(n, k, seed, ratio=10.0):
    """Gaussian spread 1 around a common per-column offset `ratio` times as large (the residual stream's common component)."""
    g = np.random.Generator(np.random.PCG64(seed))
    return (ratio * g.standard_normal((1, k)) + g.standard_normal((n, k))).astype(np.float32)


def oracle_hidden_states(p, img, heads=None):
    """Hidden states of the CPU oracle (oracle/ref_vit.py): (depth + 1, B, T, D), built from its patch_embed / block."""
    import torch
    from oracle import ref_vit
    heads = ref_vit.HEADS if heads is None else heads
    with torch.no_grad():
        B = img.shape[0]
        x = ref_vit.patch_embed(p, img)
        x = torch.cat([p["cls_token"].expand(B, -1, -1), x], dim=1) + p["pos_embed"]
        out = [x]
        for i in range(ref_vit.depth_of(p)):
            x = ref_vit.block(p, i, x, heads)
            out.append(x)
        return torch.stack(out)
