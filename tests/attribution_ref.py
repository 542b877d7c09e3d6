"""numpy / float64 restatements of csrc/attribution.hip (include/mfvit.h: mfvit_attr_inputs, mfvit_attr_accumulate, mfvit_attr_finish) and of
integrated gradients / SmoothGrad over a callable, for tests/test_attribution_{cpu,gpu}.py.

ref_*     the value in float64 (from the f32 inputs): what a kernel is compared with.
mirror_*  the kernel's own operation order in f32 numpy arithmetic (IEEE single operations, no contraction), with a `mutate` switch that
          plants one bug: the CPU tests show that the mirrors pass the gates and every mutation fails one.
gate_*    the bounds, derived from the operation orders below (U = 2^-24, the relative error of one f32 rounding; SLACK covers the
          second-order terms (1 + U)^n - 1 - n U):
  inputs      v = fmaf(alpha, fl(x - base), base): the difference carries U |x - base|, scaled by |alpha|, and the fmaf rounds once:
              |v - ref| <= U (|alpha (x - base)| + |ref|).  Without cancellation that is within 1 ulp of ref.  alpha == 0 and alpha == 1 are
              moves: exact.  With noise one more fmaf and z itself (gate_normal) add U |out| + sigma |z - z_ref|.
  normal      z = fl(sqrtf(fl(-2 logf(u1))) * cospif(fl(2 u2))): u1, u2, 2 u2 and the product by -2 are exact in f32; logf, sqrtf and cospif
              are documented at <= 1 ulp each in the HIP math tables (the gate allows 2, 1 and 2), an ulp is at most 2 U relative:
              relative error <= (2 * 2 / 2 + 2 * 1 + 2 * 2 + 1) U = 9 U (the logarithm's error halves under the root; + 1 for the product).
  accumulate  k steps a = fl(a + w_s g^p), each exact but for one rounding of a partial sum that is at most sum_s |w_s g^p| (acc starts at 0):
              <= k U sum |w g^p|.
  finish      term t_c = fl(acc_c * fl(x_c - base_c)): 2 U |t_c| (0 without times_input); pixel: C - 1 additions; patch: 8 more (2 in the
              quad, 2 across a patch row's quads, 4 across the 16 rows): <= (2 + C - 1 [+ 8]) U sum |t_c| over the pixel [patch].
  total       the f32 terms are bit-defined (IEEE operations); their double sum runs per thread (at most ~450 terms at 224 x 224) and over a
              tree 10 deep: <= 460 * 2^-53 sum |t| = 5e-14 sum |t|; the gate is 1e-12 sum |t| (SUM_TOL of the perturbation score), five
              decades below U: a single-precision sum fails it."""
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.001
SUM_TOL = 1e-12
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the noise hash
def _u32(x):
    return np.asarray(x, dtype=np.uint64) & M32


def lowbias32(x):
    x = _u32(x)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def lowbias32b(x):
    x = _u32(x)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x21f0aaad)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x735a2d97)) & M32
    x ^= x >> np.uint64(15)
    return x


def noise_key(seed, gs, b):
    seed = int(seed)
    k = lowbias32((seed & 0xFFFFFFFF) ^ int(lowbias32(((seed >> 32) + 0x9E3779B9 * (gs + 1)) & 0xFFFFFFFF)))
    return int(lowbias32((int(k) + 0x85EBCA6B * (b + 1)) & 0xFFFFFFFF))


def uniforms(seed, gs, b, n):
    """(u1, u2) of elements 0 .. n-1 of image b of global sample gs, as the kernel forms them in f32."""
    e = np.arange(n, dtype=np.uint64) ^ np.uint64(noise_key(seed, gs, b))
    h1, h2 = lowbias32(e), lowbias32b(e)
    u1 = ((h1 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u2 = (h2 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u1, u2


def ref_normal(seed, gs, b, n):
    """The standard normals of the kernel's definition in float64 (from its f32 uniforms)."""
    u1, u2 = uniforms(seed, gs, b, n)
    t = 2.0 * u2.astype(np.float64)
    c = np.cos(np.pi * t)
    c[(t == 0.5) | (t == 1.5)] = 0.0                               # cospi is exact there
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * c


def ref_noise(seed, s0, S, shape):
    """z of samples s0 .. s0 + S - 1 for images of `shape` (B, C, H, W): float64 (S, B, C, H, W)."""
    B, n = shape[0], int(np.prod(shape[1:]))
    return np.stack([np.stack([ref_normal(seed, s0 + s, b, n) for b in range(B)]) for s in range(S)]).reshape((S,) + tuple(shape))


def gate_normal(z_ref):
    return 9 * U * SLACK * np.abs(z_ref) + 1e-30


# ------------------------------------------------------------------------------------------------ inputs
def _base_like(base, x):
    base = np.asarray(base)
    return base.reshape(1, -1, 1, 1) + np.zeros_like(x) if base.ndim == 1 else base


def ref_inputs(x, base, alpha, sigma=None, z=None):
    """float64 (S, B, C, H, W) from f32 x, base ((C,) or full), alpha (S,), sigma (B,), z float64 (S, B, C, H, W)."""
    x64, b64 = x.astype(np.float64), _base_like(base, x).astype(np.float64)
    out = b64[None] + alpha.astype(np.float64).reshape(-1, 1, 1, 1, 1) * (x64 - b64)[None]
    if sigma is not None:
        out = out + sigma.astype(np.float64).reshape(1, -1, 1, 1, 1) * z
    return out


def gate_inputs(x, base, alpha, ref, sigma=None, z=None):
    d = np.abs(x.astype(np.float64) - _base_like(base, x).astype(np.float64))
    g = U * SLACK * (np.abs(alpha.astype(np.float64)).reshape(-1, 1, 1, 1, 1) * d[None] + np.abs(ref))
    g[(alpha == 0) | (alpha == 1)] = 0.0                           # moves
    if sigma is not None:
        g = g + U * SLACK * np.abs(ref) + np.abs(sigma.astype(np.float64)).reshape(1, -1, 1, 1, 1) * gate_normal(z)
    return g


def mirror_inputs(x, base, alpha, mutate=None):
    """The noise-free kernel in f32 numpy arithmetic.  (The fmaf is formed in float64 and rounded once: alpha * d is exact there.)"""
    b = _base_like(base, x).astype(np.float32)
    d = (x - b).astype(np.float32)
    out = np.empty((len(alpha),) + x.shape, np.float32)
    for s, a in enumerate(alpha):
        v = (np.float64(a) * d.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
        out[s] = b if a == 0 else (x if a == 1 else v)
    if mutate == "skip_second_group":                              # elements 4 .. 7 of every image row keep what the buffer held
        out[..., 4:8] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ accumulate
def ref_accumulate(g, w, power):
    return np.tensordot(w.astype(np.float64), g.astype(np.float64) ** power, axes=(0, 0))


def gate_accumulate(g, w, power):
    k = g.shape[0]
    return k * U * SLACK * np.tensordot(np.abs(w.astype(np.float64)), np.abs(g.astype(np.float64)) ** power, axes=(0, 0))


def mirror_accumulate(g, w, power, mutate=None):
    a = np.zeros(g.shape[1:], np.float32)
    k = g.shape[0] - 1 if mutate == "drop_last_step" else g.shape[0]
    for s in range(k):
        a = (np.float64(w[s]) * g[s].astype(np.float64) ** power + a.astype(np.float64)).astype(np.float32)
    if mutate == "skip_second_group":
        a.reshape(a.shape[0], -1)[:, 4:8] = 0.0
    return a


# ------------------------------------------------------------------------------------------------ finish
def _patch_sum(p):
    B, H, W = p.shape
    return p.reshape(B, H // 16, 16, W // 16, 16).sum(axis=(2, 4))


def ref_finish(acc, x=None, base=None, absval=False):
    """float64: (pixels (B, H, W), patches (B, gh, gw), total (B,), abs-term sums per pixel, per patch)."""
    t = acc.astype(np.float64)
    if x is not None:
        t = t * (x.astype(np.float64) - _base_like(base, x).astype(np.float64))
    px = (np.abs(t) if absval else t).sum(axis=1)
    mag = np.abs(t).sum(axis=1)
    return px, _patch_sum(px), t.sum(axis=(1, 2, 3)), mag, _patch_sum(mag)


def gate_finish(C, times_input, mag_pixel, mag_patch):
    n = (2 if times_input else 0) + C - 1
    return n * U * SLACK * mag_pixel, (n + 8) * U * SLACK * mag_patch


def f32_terms(acc, x=None, base=None):
    """The kernel's f32 terms t_c, bit for bit (IEEE single operations)."""
    if x is None:
        return acc.astype(np.float32)
    return (acc * (x - _base_like(base, x).astype(np.float32)).astype(np.float32)).astype(np.float32)


def exact_total(terms):
    return np.array([math.fsum(t.reshape(-1).astype(np.float64).tolist()) for t in terms]), np.abs(terms.astype(np.float64)).sum(axis=(1, 2, 3))


def mirror_finish(acc, x=None, base=None, absval=False, mutate=None):
    """The kernel's summation tree in f32: (pixels, patches, total)."""
    t = f32_terms(acc, x, base)
    B, C, H, W = t.shape
    f = np.abs(t) if absval else t
    nc = C - 1 if mutate == "drop_channel" and C > 1 else C
    px = f[:, 0].copy()
    for c in range(1, nc):
        px = (px + f[:, c]).astype(np.float32)
    v = px.reshape(B, H // 16, 16, W // 16, 4, 4)                  # (b, py, r, px, quad, pixel)
    if mutate == "drop_col":
        v = v.copy(); v[..., 3, 3] = 0.0
    q = ((v[..., 0] + v[..., 1]).astype(np.float32) + (v[..., 2] + v[..., 3]).astype(np.float32)).astype(np.float32)
    rows = ((q[..., 0] + q[..., 1]).astype(np.float32) + (q[..., 2] + q[..., 3]).astype(np.float32)).astype(np.float32)   # (b, py, r, px)
    rs = [rows[:, :, r] for r in range(15 if mutate == "drop_row" else 16)] + ([np.zeros_like(rows[:, :, 0])] if mutate == "drop_row" else [])
    while len(rs) > 1:
        rs = [(rs[i] + rs[i + 1]).astype(np.float32) for i in range(0, len(rs), 2)]
    if mutate == "f32_total":
        total = t.reshape(B, -1).astype(np.float32).cumsum(axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    else:
        total = exact_total(t)[0]
    return px, rs[0], total


# ------------------------------------------------------------------------------------------------ the methods over a callable, float64
def path_points(steps, rule):
    if rule == "trapezoid":
        return [i / steps for i in range(steps + 1)], [(0.5 if i in (0, steps) else 1.0) / steps for i in range(steps + 1)]
    return [(i + 0.5) / steps for i in range(steps)], [1.0 / steps] * steps


def integrated_gradients(score_and_grad, x, base, alphas, weights):
    """(attribution, score(x), score(base)) for score_and_grad(points) -> (scores (B,), gradients like points): float64 arrays."""
    acc = np.zeros_like(x)
    for a, w in zip(alphas, weights):
        acc += w * score_and_grad(base + a * (x - base))[1]
    return (x - base) * acc, score_and_grad(x)[0], score_and_grad(base)[0]


def smoothgrad(score_and_grad, x, noise, squared=False):
    """The mean gradient (or squared gradient) over the noisy copies x + noise[s]."""
    acc = np.zeros_like(x)
    for n in noise:
        g = score_and_grad(x + n)[1]
        acc += (g * g if squared else g) / len(noise)
    return acc
