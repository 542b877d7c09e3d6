"""float64 restatement of the per-head attention statistics (include/mfvit.h, mfvit_attention_stats), their gate, and the single-op cases
shared by tests/test_attnstats_cpu.py and tests/test_attnstats_gpu.py.

Definitions, per head, for the T x T softmax P with T = 1 + gh * gw (token 0: cls; patch token i >= 1 at divmod(i - 1, gw)) and
d_ij = patch * sqrt((y_i - y_j)^2 + (x_i - x_j)^2):
  0 distance         (1/(T-1)) sum_{i>=1} sum_{j>=1} P_ij d_ij
  1 distance_renorm  (1/(T-1)) sum_{i>=1} (sum_{j>=1} P_ij d_ij) / (sum_{j>=1} P_ij)
  2 entropy          (1/T) sum_i H(P_i),  H(P_i) = -sum_j P_ij ln P_ij
  3 cls_entropy      H(P_0)
  4 cls_mass         (1/(T-1)) sum_{i>=1} P_i0
  5 self_mass        (1/T) sum_i P_ii

Gate.  gate(T, ref, scale) = (T + 16) * 2^-24 * (|ref| + scale), scale = patch for the two distances and 1 for the rest, doubled for
distance_renorm (two sums and a quotient).  Every term of a row sum is non-negative, so f32 summation of at most T terms in ANY order has a
relative error of at most T u (u = 2^-24); a few u more come from the product, the square root and the exponential; from the rows upward the
kernel adds in double.  A CPU simulation with sequential f32 accumulation (f32_floor below; test_attnstats_cpu.py) stays far inside it.
"""
import numpy as np

STATS = ("distance", "distance_renorm", "entropy", "cls_entropy", "cls_mass", "self_mass")
U = 2.0 ** -24
F32, BF16, BF16X3, F16, X3F16 = 0, 1, 2, 3, 4

# single-op cases: (storage tag, gh, gw, B, H, head_dim); in every one q is Gaussian with standard deviation 1 and k with standard deviation 3
# (STD_Q, STD_K), so that the scores scale q.k / sqrt(head_dim) have standard deviation 3 - the largest score scale the gate's derivation
# covers.  Every format at 14 x 14; f32 and split bf16 at one patch (T = 2), T = 5, one tile + 1 (33), 65, wave 0's second key tile (129), a
# non-square grid (201) and several strides per wave (577); B in {1, 3}, H in {1, 3, 12}, head_dim 32 / 64 / 96 spread over them (f32
# attention has no head_dim 96, split fp16 only 32).
STD_Q, STD_K = 1.0, 3.0
CASES = [
    (F32, 14, 14, 1, 3, 64), (BF16, 14, 14, 3, 1, 32), (F16, 14, 14, 1, 12, 32), (BF16X3, 14, 14, 1, 3, 96), (X3F16, 14, 14, 3, 3, 32),
    (F32, 1, 1, 3, 12, 32), (BF16X3, 1, 1, 1, 1, 96),
    (F32, 2, 2, 1, 1, 64), (BF16X3, 2, 2, 3, 3, 32),
    (F32, 4, 8, 1, 3, 32), (BF16X3, 4, 8, 1, 12, 64),
    (F32, 8, 8, 3, 1, 64), (BF16X3, 8, 8, 1, 3, 96),
    (F32, 8, 16, 1, 3, 64), (BF16X3, 8, 16, 3, 1, 32),
    (F32, 10, 20, 1, 12, 32), (BF16X3, 10, 20, 1, 3, 64),
    (F32, 24, 24, 1, 3, 32), (BF16X3, 24, 24, 1, 1, 96),
]


def case_id(c):
    return f"{('f32', 'bf16', 'bf16x3', 'f16', 'x3f16')[c[0]]}-{c[1]}x{c[2]}-B{c[3]}-H{c[4]}-hd{c[5]}"


def distances(gh, gw, patch=16.0):
    """(T, T) float64 d_ij; row and column 0 (cls) are zero and unused."""
    y, x = np.divmod(np.arange(gh * gw), gw)
    d = np.zeros((gh * gw + 1, gh * gw + 1))
    d[1:, 1:] = patch * np.sqrt(((y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2).astype(np.float64))
    return d


def entropy_rows(P):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(P > 0, P * np.log(P), 0.0).sum(axis=-1)


def stats(P, gh, gw, patch=16.0):
    """(..., T, T) probabilities -> (..., 6) float64 statistics."""
    P = np.asarray(P, dtype=np.float64)
    T = gh * gw + 1
    assert P.shape[-2:] == (T, T)
    d = distances(gh, gw, patch)
    pd = (P[..., 1:, 1:] * d[1:, 1:]).sum(axis=-1)                   # (..., T - 1)
    ps = P[..., 1:, 1:].sum(axis=-1)
    H = entropy_rows(P)                                              # (..., T)
    out = np.empty(P.shape[:-2] + (6,))
    out[..., 0] = pd.sum(axis=-1) / (T - 1)
    out[..., 1] = (pd / ps).sum(axis=-1) / (T - 1)
    out[..., 2] = H.sum(axis=-1) / T
    out[..., 3] = H[..., 0]
    out[..., 4] = P[..., 1:, 0].sum(axis=-1) / (T - 1)
    out[..., 5] = np.diagonal(P, axis1=-2, axis2=-1).sum(axis=-1) / T
    return out


def scales(patch=16.0):
    return np.array([patch, patch, 1.0, 1.0, 1.0, 1.0])


def gate(T, ref, scale):
    return (T + 16) * U * (np.abs(ref) + scale)


def gates(T, ref, patch=16.0):
    """The gate of every element of a (..., 6) reference: gate(T, ref, scale), doubled for distance_renorm."""
    g = gate(T, np.asarray(ref, dtype=np.float64), scales(patch))
    g[..., 1] *= 2.0
    return g


def gaussian_qk(seed, B, T, H, hd, std_q=STD_Q, std_k=STD_K):
    """float64 (B, T, 3, H, hd) qkv with Gaussian q and k of the given standard deviations (v: unit)."""
    g = np.random.Generator(np.random.PCG64(seed))
    qkv = g.standard_normal((B, T, 3, H, hd))
    qkv[:, :, 0] *= std_q
    qkv[:, :, 1] *= std_k
    return qkv


def probs_from_qk(qkv, lse=None):
    """float64 P (B, H, T, T) = exp(scale q.k - lse) of a (B, T, 3, H, hd) array; lse (B, H, T) natural log, or None for the exact one."""
    q = np.transpose(qkv[:, :, 0], (0, 2, 1, 3)).astype(np.float64)
    k = np.transpose(qkv[:, :, 1], (0, 2, 1, 3)).astype(np.float64)
    s = np.einsum("bhid,bhjd->bhij", q, k) * qkv.shape[-1] ** -0.5
    if lse is None:
        m = s.max(axis=-1, keepdims=True)
        lse = (m + np.log(np.exp(s - m).sum(axis=-1, keepdims=True)))[..., 0]
    return np.exp(s - np.asarray(lse, dtype=np.float64)[..., None])


def f32_floor(P, gh, gw, patch=16.0):
    """The statistics as an honest f32 kernel would form them: P, d and log2 P rounded to f32, f32 products, every row sum accumulated
    SEQUENTIALLY in f32 (np.cumsum does not pair), the rows upward in double."""
    T = gh * gw + 1
    P32 = np.asarray(P, dtype=np.float64).astype(np.float32)
    d32 = distances(gh, gw, 1.0).astype(np.float32)
    d32 = (np.float32(patch) * np.sqrt((d32 * d32).round().astype(np.float32))).astype(np.float32)
    with np.errstate(divide="ignore"):
        e32 = np.log2(np.asarray(P, dtype=np.float64)).astype(np.float32)

    def rowsum(a):
        return np.cumsum(a.astype(np.float32), axis=-1, dtype=np.float32)[..., -1].astype(np.float64)
    pd = rowsum(P32[..., 1:, 1:] * d32[1:, 1:])
    ps = rowsum(P32[..., 1:, 1:])
    H = rowsum(np.where(P32 > 0, P32 * -e32, np.float32(0))) * np.log(2.0)
    out = np.empty(P32.shape[:-2] + (6,))
    out[..., 0] = pd.sum(axis=-1) / (T - 1)
    out[..., 1] = (pd / ps).sum(axis=-1) / (T - 1)
    out[..., 2] = H.sum(axis=-1) / T
    out[..., 3] = H[..., 0]
    out[..., 4] = P32[..., 1:, 0].astype(np.float64).sum(axis=-1) / (T - 1)
    out[..., 5] = np.diagonal(P32, axis1=-2, axis2=-1).astype(np.float64).sum(axis=-1) / T
    return out


def x4_params(sd, factor=4.0):
    """A copy of an encoder state dict whose q and k rows of every attn.qkv.weight are multiplied by `factor`: the seeded weights give
    near-uniform attention whose heads differ by a few per cent; sharper scores make the heads distinct ((max - min) / mean of `distance` over
    the heads of a block: 11 - 12 % at factor 4 on the images of the tests, a few per cent unscaled), so that a head or block mix-up cannot hide under a 16-bit gate."""
    out = {k: v.clone() for k, v in sd.items()}
    for k, v in out.items():
        if k.endswith("attn.qkv.weight"):
            D = v.shape[1]
            v[:2 * D] *= factor
    return out
