"""Test helper: float64 restatement of SAM / ASAM (first_step / second_step of davda54/sam's wrapper, written from the papers' formulae), the
gates of the SAM kernels (csrc/optim.hip: sam_norm_adaptive_kernel, sam_scale_kernel, sam_perturb_kernel, sam_restore_kernel), a float32
restatement of the adaptive norm's row split and of the element-wise pass, both with mutations, and the input builders.
tests/test_sam_cpu.py pins the restatement to a per-tensor torch SAM and shows that the gates catch the mutations; tests/test_sam_gpu.py
compares the kernels with it.

Formulae.  SAM (Foret et al. 2021, eq. 2 / algorithm 1):  e = rho g / |g|_2, the norm over ALL gradients.  ASAM (Kwon et al. 2021, eq. 8 with
T_w = |w| element-wise):  e = rho T_w^2 g / |T_w g|_2 = rho w^2 g / | |w| g |_2.  davda54's code adds 1e-12 to the norm and takes rho per param
group while the norm stays one number:  scale_group = rho_group / (norm + 1e-12),  w <- w + e  (first_step),  w <- old w, then the base
optimizer's step on the gradients taken at w + e  (second_step).

Gates: derived, not measured (first order in u = 2^-24, as in grad_clip_ref.py).  The plain norm pass IS grad_norm_kernel<0>: D = 44 roundings on
the way of an addend into a row's sum of squares (grad_clip_ref.py).  The adaptive pass has the same split and order with the addend t^2,
t = fl(|w| g): t carries one rounding, its square two (the square itself is not rounded: it goes into the fmaf), so
    D_A = D + 2 = 46
and a total that mixes plain and adaptive groups is covered by D_A.  Everything behind the row partials runs in double (sam_scale_kernel):
    total norm              (D_A / 2 + 1) u = 1.43e-6   (half the error of the sum through the sqrt, one rounding to float)
    inv = 1 / (norm + 1e-12) (D_A / 2 + 1) u            (the same error through the reciprocal - the 1e-12 only shrinks it - and one rounding)
both relative, atol 0.  The element-wise pass is compared for BITS with a float32 restatement that is fed the device's own inv.  Against
float64, e = g s with s = fl(rho inv) is off by (D_A / 2 + 1) + 1 + 1 roundings, an adaptive e = fl(fl(fl(w w) g) s) by two more, and
w + e is rounded once relative to the result:
    |w' - w'_64| <= E_RTOL |e| + u |w'|,   E_RTOL = (D_A / 2 + 5) u = 1.67e-6
"""
import math

import torch

import grad_clip_ref as gref
from grad_clip_ref import CHUNK, U, boosted, rel_ratio  # noqa: F401  (re-exported)

D_A = gref.D + 2
NORM_RTOL = (D_A / 2 + 1) * U
INV_RTOL = (D_A / 2 + 1) * U
E_RTOL = (D_A / 2 + 5) * U
assert D_A == 46 and NORM_RTOL <= 1.5e-6 and E_RTOL <= 1.7e-6
NORM_MUTATIONS = gref.MUTATIONS                                  # skip_head, skip_tail, drop_second_group
ELEM_MUTATIONS = ("skip_head", "skip_tail", "forget_ww")
# every size edge of the head / 16-byte group / tail split: 1024 +- 1 (a full first sweep of 256 groups), 1028 / 1029 (the second accumulator's first
# group), 2048 +- 1 (the second accumulator's full sweep), the row boundary, a tensor over four rows
COUNTS = (1, 3, 4, 5, 255, 1023, 1024, 1025, 1028, 1029, 2047, 2048, 2049, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)


# ------------------------------------------------------------------------------------------------ float64
def sam_norm_ref(ws, gs, adaptives):
    """The one norm of first_step over tensors with their group's `adaptive`, float64."""
    sq = torch.zeros((), dtype=torch.float64)
    for w, g, a in zip(ws, gs, adaptives):
        t = (w.double().abs() if a else 1.0) * g.double()
        sq = sq + t.square().sum()
    return sq.sqrt()


def first_step_ref(ws, gs, rhos, adaptives):
    """(norm, inv, e per tensor, perturbed w per tensor), float64.  A non-finite norm moves nothing (inv 0): the wrapper's overflow rule."""
    norm = sam_norm_ref(ws, gs, adaptives)
    inv = 1.0 / (norm + 1e-12) if bool(torch.isfinite(norm)) else torch.zeros((), dtype=torch.float64)
    es = [(w.double().square() if a else 1.0) * g.double() * (r * inv) for w, g, r, a in zip(ws, gs, rhos, adaptives)]
    return norm, inv, es, [w.double() + e for w, e in zip(ws, es)]


def second_step_ref(old_ws, base_step):
    """w <- old w, then the base optimizer: base_step(i, w) -> the float64 reference step of tensor i (oracle/ref_optim.py)."""
    return [base_step(i, w) for i, w in enumerate(old_ws)]


def perturbed_ratio(got, w_ref, e_ref):
    """max |got - w'| / (E_RTOL |e| + u |w'|): <= 1 passes."""
    got, w_ref, e_ref = (t.double().cpu().flatten() for t in (got, w_ref, e_ref))
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err, den = (got - w_ref).abs(), E_RTOL * e_ref.abs() + U * w_ref.abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / den)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ inputs
def inputs(counts=COUNTS, seed=8800):
    """(w list, g list): N(0, 1), the first and last three elements of each pushed to magnitude >= 1 (grad_clip_ref.boosted), so that no edge element
    a mutation drops is small - neither in g nor in |w| g."""
    from conftest import rng_tensor
    ws = [boosted(rng_tensor(seed + i, (c,))) for i, c in enumerate(counts)]
    gs = [boosted(rng_tensor(seed + 500 + i, (c,))) for i, c in enumerate(counts)]
    return ws, gs


# ------------------------------------------------------------------------------------------------ float32 restatements
def adaptive_norm_sq_f32(w, g, phase, mutate=None):
    """Sum of squares sam_norm_adaptive_kernel + sam_scale_kernel give for one tensor in rows of CHUNK whose GRADIENT starts `phase` floats behind
    a 16-byte boundary: t = fl(|w| g), then grad_norm_kernel<0>'s split and order on t (grad_clip_ref.row_partial_f32), the rows in double.
    Returns (sum as a Python float, whether the mutation dropped anything)."""
    t = w.float().abs() * g.float()
    acc, dropped = 0.0, False
    for a in range(0, t.numel(), CHUNK):
        p, d = gref.row_partial_f32(t[a:a + CHUNK], phase, mutate)
        acc += float(p)
        dropped |= d
    return acc, dropped


def perturb_f32(w, g, inv, rho, adaptive, phase=0, mutate=None):
    """sam_perturb_kernel on one row in float32, every operation rounded on its own: s = rho * inv; e = g * s or ((w * w) * g) * s; w + e.  `inv` is
    the device's float32 value, `rho` the float the C ABI carries.  Mutations: the head (up to the 16-byte boundary `phase` floats before the
    row) or the tail (behind the last full group) is not updated; the adaptive e forgets w * w."""
    f = torch.float32
    w, g = w.to(f), g.to(f)
    s = torch.tensor(rho, dtype=f) * torch.tensor(inv, dtype=f)
    e = ((w * w) * g) * s if adaptive and mutate != "forget_ww" else g * s
    out = w + e
    n = w.numel()
    head = min((4 - phase) % 4, n)
    ntail = (n - head) % 4
    if mutate == "skip_head" and head:
        out[:head] = w[:head]
    if mutate == "skip_tail" and ntail:
        out[n - ntail:] = w[n - ntail:]
    return out
