"""Oracle: single optimizer steps in float64, written from the formulas csrc/optim.hip cites.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Pinned to torch.optim.Adam / AdamW / SGD (float64, CPU) and to the reference's LARS
trajectory (tests/golden/lars.npz) by tests/test_step_refs_cpu.py; the references of tests/test_optim_kernels_gpu.py.

  LARS          moco/optimizer.py:10-43 of the reference: weight decay and trust ratio only for tensors with ndim > 1, q = 1 when either norm is 0
  Adam / AdamW  torch.optim semantics with a per-parameter `step` (the value AFTER the increment: 1 for the first step)
  SGD           torch.optim.SGD with momentum and L2 weight decay, no dampening / nesterov: the first step stores d as the buffer
  AMP unscale   GradScaler.unscale_: g * inv_scale, found_inf iff an element is not finite BEFORE the scaling

Every function widens its inputs to float64 and returns new tensors.
"""
import torch


def lars_step(p, g, mu, lr, weight_decay=0.0, momentum=0.9, trust_coefficient=0.001, ndim=None):
    """One tensor.  `ndim`: the parameter's ndim when `p` is handed in flattened.  Returns (p, mu)."""
    p, dp, mu = p.double(), g.double(), mu.double()
    if (p.ndim if ndim is None else ndim) > 1:
        dp = dp + weight_decay * p
        pn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(dp)
        q = trust_coefficient * pn / un if (pn > 0 and un > 0) else 1.0
        dp = dp * q
    mu = mu * momentum + dp
    return p - lr * mu, mu


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False):
    """Returns (p, exp_avg, exp_avg_sq).  decoupled: AdamW (p *= 1 - lr wd) instead of Adam (g += wd p)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


def sgd_step(p, g, buf, lr, momentum=0.0, weight_decay=0.0, first_step=False):
    """Returns (p, momentum buffer); with momentum == 0 the buffer is handed back untouched (None stays None)."""
    p, d = p.double(), g.double()
    d = d + weight_decay * p
    if momentum != 0:
        d = d if first_step else momentum * buf.double() + d
        buf = d
    return p - lr * d, buf


def amp_unscale(g, inv_scale):
    """Returns (g * inv_scale, found_inf)."""
    return g.double() * inv_scale, bool((~torch.isfinite(g)).any())


# ------------------------------------------------------------------------------------------------ the size / alignment matrix of adam_kernel
# Shared by the GPU test and the CPU mutation check.  adam_kernel (csrc/optim.hip) takes, per chunk-table row of `count` elements: with all of
# p / g / m / v on 16-byte boundaries, float4 groups i and i + 256 per thread at stride 512 (the second one only when it exists), then a scalar
# tail of count % 4 elements; with any pointer off a boundary, scalar accesses throughout.
ADAM_N4 = (0, 1, 255, 256, 257, 511, 512, 513, 4096)
ADAM_R = (0, 1, 3)
ADAM_COUNTS = tuple(4 * n4 + r for n4 in ADAM_N4 for r in ADAM_R if 4 * n4 + r > 0)
ADAM_ALIGN = ("aligned", "p", "g", "m", "v", "all")        # which of the four pointers sit one..three floats off a 16-byte boundary
ADAM_MUTATIONS = ("drop_second", "skip_tail")
ADAM_PATHS = ("vector_single", "vector_pair", "tail", "scalar")


def adam_path_of(count, aligned):
    """(count,) int8 path index into ADAM_PATHS of every element of one table row."""
    i = torch.arange(count)
    if not aligned:
        return torch.full((count,), 3, dtype=torch.int8)
    n4 = count // 4
    grp = i // 4
    first = grp % 512 < 256
    paired = torch.where(first, grp + 256 < n4, torch.ones_like(first))          # a second group exists only as part of a pair
    path = torch.where(paired, torch.ones_like(grp), torch.zeros_like(grp))
    path = torch.where(i >= 4 * n4, torch.full_like(grp, 2), path)
    return path.to(torch.int8)


def adam_split_f32(p, g, m, v, aligned, step, lr, beta1, beta2, eps, weight_decay, decoupled, mutate=None):
    """float32 restatement of one adam_kernel table row with its vector / pair / tail split.  Returns (p, m, v, reached).  `mutate`:
      drop_second   the second float4 group of a pair (i + 256) is never updated
      skip_tail     the scalar tail behind the float4 groups is never updated"""
    f = torch.float32
    p, g, m, v = p.to(f), g.to(f), m.to(f), v.to(f)
    c = lambda x: torch.tensor(x, dtype=f)      # noqa: E731  (the kernel's constants are floats)
    lr_, b1, b2, eps_, wd = c(lr), c(beta1), c(beta2), c(eps), c(weight_decay)
    bc1 = 1 - b1 ** step
    bc2s = (1 - b2 ** step).sqrt()
    pn, gn = (p * (1 - lr_ * wd), g) if decoupled else (p, wd * p + g)
    mn = b1 * m + (1 - b1) * gn
    vn = b2 * v + (1 - b2) * gn * gn
    pn = pn - (lr_ / bc1) * mn / (vn.sqrt() / bc2s + eps_)
    path = adam_path_of(p.numel(), aligned)
    grp = torch.arange(p.numel()) // 4
    keep = torch.zeros(p.numel(), dtype=torch.bool)
    if mutate == "drop_second":
        keep = (path == 1) & (grp % 512 >= 256)
    elif mutate == "skip_tail":
        keep = path == 2
    return torch.where(keep, p, pn), torch.where(keep, m, mn), torch.where(keep, v, vn), bool(keep.any())


def gate_ratio(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): <= 1 passes a torch.testing.assert_close gate; NaN counts as infinite."""
    got, ref = got.double().cpu(), ref.double().cpu()
    r = ((got - ref).abs() / (atol + rtol * ref.abs())).max()
    return float("inf") if bool(torch.isnan(r)) else float(r)
