"""Test helper: float64 restatement of torch.nn.utils.clip_grad_norm_ (norm_ref, clip_ref), the gates of the gradient-clipping kernels
(csrc/optim.hip: grad_norm_kernel, grad_clip_coef_kernel, grad_scale_kernel) and a float32 restatement of the norm pass's row split with
mutations.  tests/test_grad_clip_cpu.py pins the restatement to torch and shows that the gate catches a dropped head, tail or second group;
tests/test_grad_clip_gpu.py compares the kernels with it.

The gate is derived, not measured.  D is the longest chain of float32 roundings an addend of a row's sum of squares passes through in
grad_norm_kernel, for a table row of at most CHUNK = 16,384 elements (the rows mfvit.optim builds):
    head element            1   (s0 = g * g)
    16-byte groups         32   (at most 4,096 groups per row / 256 threads / 2 accumulators = 8 groups of 4 fmaf steps per accumulator;
                                 the tail element's single fmaf on s1 stands where s0 has its head element: 33 per accumulator at most)
    s0 + s1                 1
    wave_sum                6   (shuffle levels)
    the 4 wave sums         4   (block_sum adds them to 0.f in order)
                     D = 44
Everything after that (row partials -> per-tensor and total sums, sqrt, the coefficient) runs in double and is rounded to float32 once.
With u = 2^-24 and all terms non-negative, the sum of squares is off by at most D u relative, so
    a norm (per tensor or total)   is off by at most (D / 2 + 1) u   (half the error of the sum through the sqrt, one rounding of the result)
    a scaled gradient              by at most         (D / 2 + 3) u   (the coefficient: D / 2 from the total, one rounding; the product: one more;
                                                                        the 1e-6 of the formula is the same number on both sides)
Both gates are purely relative (atol 0).  The inf norm is a maximum: exact, compared for equality.
"""
import math

import torch

CHUNK = 1 << 14
D = 44
U = 2.0 ** -24
NORM_RTOL = (D / 2 + 1) * U         # 1.37e-6
GRAD_RTOL = (D / 2 + 3) * U         # 1.49e-6
assert D <= 96 and GRAD_RTOL <= 3e-6
MUTATIONS = ("skip_head", "skip_tail", "drop_second_group")


def _kind(norm_type):
    nt = float(norm_type)
    assert nt in (2.0, math.inf)
    return nt


def norm_ref(grads, norm_type=2.0):
    """(per-tensor norms, total) in float64 of a list of tensors."""
    nt = _kind(norm_type)
    per = torch.stack([torch.linalg.vector_norm(g.double().flatten(), nt) if g.numel() else torch.zeros((), dtype=torch.float64) for g in grads])
    return per, torch.linalg.vector_norm(per, nt)


def clip_ref(grads, max_norm, norm_type=2.0):
    """(total, coef, per-tensor norms, clipped gradients), float64: coef = min(1, max_norm / (total + 1e-6)), a NaN total gives a NaN coef."""
    per, total = norm_ref(grads, norm_type)
    coef = torch.clamp(float(max_norm) / (total + 1e-6), max=1.0)
    return total, coef, per, [g.double() * coef for g in grads]


def rel_ratio(got, ref, rtol):
    """max |got - ref| / (rtol |ref|) (atol 0; 0 vs 0 counts as 0): <= 1 passes.  NaN or inf anywhere counts as infinite."""
    got, ref = got.double().cpu().flatten(), ref.double().cpu().flatten()
    if not bool(torch.isfinite(got).all() and torch.isfinite(ref).all()):
        return math.inf
    err, den = (got - ref).abs(), rtol * ref.abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / den)
    return float(r.max()) if r.numel() else 0.0


def boosted(x):
    """The input condition of the mutation check: the first and last three elements of a view become sign(x) (1 + |x|), so that no edge element
    the row split could drop is small.  A tensor of n ~ N(0, 1) elements has a sum of squares of about n, and an element of magnitude >= 1 that is
    dropped moves its norm by at least 1 / (2 n): 1e-5 for the largest tensor used (3 CHUNK + 5 = 49,157 elements), seven times the gate."""
    x = x.clone()
    idx = sorted(set(list(range(min(3, x.numel()))) + list(range(max(0, x.numel() - 3), x.numel()))))
    e = x[idx]
    x[idx] = torch.where(e < 0, -torch.ones_like(e), torch.ones_like(e)) * (1 + e.abs())
    return x


def inputs(counts, seed=7700):
    from conftest import rng_tensor
    return [boosted(rng_tensor(seed + i, (c,))) for i, c in enumerate(counts)]


# ------------------------------------------------------------------------------------------------ float32 restatement of the norm pass
def _fma_sq(x, s):
    """float32 fmaf(x, x, s): the square of a float32 is exact in float64."""
    return (s.double() + x.double() * x.double()).float()


def row_partial_f32(g, phase, mutate=None):
    """The sum of squares grad_norm_kernel writes for one table row `g` (float32, <= CHUNK elements) that starts `phase` floats behind a 16-byte
    boundary, in the kernel's order.  Returns (partial as a float32 0-dim tensor, whether the mutation dropped anything)."""
    f = torch.float32
    g = g.to(f)
    n = g.numel()
    head = min((4 - phase) % 4, n)
    n4 = (n - head) // 4
    ntail = n - head - 4 * n4
    s0, s1 = torch.zeros(256, dtype=f), torch.zeros(256, dtype=f)
    dropped = False
    if head:
        if mutate == "skip_head":
            dropped = True
        else:
            s0[:head] = g[:head] * g[:head]
    iters = (n4 + 511) // 512
    body = torch.zeros(iters * 512 * 4, dtype=f)            # groups that do not exist add 0 * 0: exact
    body[:4 * n4] = g[head:head + 4 * n4]
    body = body.view(iters, 2, 256, 4)
    for it in range(iters):
        for k in range(4):
            s0 = _fma_sq(body[it, 0, :, k], s0)
        if mutate == "drop_second_group":
            dropped |= n4 > it * 512 + 256
            continue
        for k in range(4):
            s1 = _fma_sq(body[it, 1, :, k], s1)
    if ntail:
        if mutate == "skip_tail":
            dropped = True
        else:
            s1[:ntail] = _fma_sq(g[n - ntail:], s1[:ntail])
    v = (s0 + s1).view(4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):                          # wave_sum: v += shfl_xor(v, o)
        v = v + v[:, lane ^ o]
    t = torch.zeros((), dtype=f)
    for w in range(4):                                       # block_sum: the wave sums in order
        t = t + v[w, 0]
    return t, dropped


def tensor_norm_f32(g, phase, mutate=None):
    """L2 norm of one tensor laid out in table rows of CHUNK elements (CHUNK % 4 == 0: every row has the tensor's phase): the row partials of
    row_partial_f32 summed in double in row order, as grad_clip_coef_kernel does.  Returns (norm as float64, dropped)."""
    acc, dropped = 0.0, False
    for a in range(0, g.numel(), CHUNK):
        p, d = row_partial_f32(g[a:a + CHUNK], phase, mutate)
        acc += float(p)
        dropped |= d
    return math.sqrt(acc), dropped
