"""The two small cross entropies (C <= 64 classes) through the C ABI against float64 on the same float32 logits:
  mfvit_cross_entropy        ce_small_kernel, csrc/elementwise.hip - against torch.nn.functional.cross_entropy and its autograd gradient
  mfvit_cross_entropy_soft   ce_soft_kernel, csrc/mix.hip - against the float64 oracle of tests/test_mixup_gpu.py, with and without partner / lam
Both stride the samples over ONE block of 1,024 threads and add the row losses in a fixed order.  tests/test_ops_gpu.py and tests/test_mixup_gpu.py
stop at B = 257: here B runs below, at and past 1,024 and into a third trip (2,500), C from 1 to the limit 64, the logits at scale 1 and at scale
30 (saturated rows: the right class carries a tiny loss beside row losses of 100 and more), targets in column 0 and C - 1, exact ties at the row
maximum, dlogits NULL, preds NULL.  Every buffer is a view inside a NaN-filled (integers: sentinel-filled) tensor: a read of a neighbour poisons the
result, a write outside the window is seen bit for bit, inputs are compared afterwards.  Targets stay inside [0, C): these kernels index the row
with them.  Measured errors are appended to parity_ops.txt; tests/test_step_refs_cpu.py prints the CPU floor of the gate."""
import numpy as np
import pytest
import torch

from oracle import ref_moco

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
NAN = float("nan")
SENTINEL = -0x0123456789ABCDEF
EINVAL = -22

# Gate on the loss and on dlogits of both kernels, by the recipe above CE_GATE in tests/test_moco_rowops_gpu.py (the same __expf / __logf arithmetic;
# its ceiling 2e-5 is the ceiling here).
#   measure   loss: |error| over |loss| at scale 1; at scale 30 over the batch's largest row loss (the mean of saturated rows is dominated by the few
#             wrong ones: it is their size the float32 sum is held to).  dlogits: max |error| over 1 / B, the size of (softmax - y) / B - the
#             tensor's own max abs is arbitrarily small where every row is saturated on its target.
#   floor     float32 restatement with exact exp / log (oracle/ref_moco.py::ce_small_f32) over the matrix, on the CPU: loss 6.0e-8, dlogits 3.9e-6
#             (exp(z - lse) with lse rounded to float32 at |lse| up to 150: 2^-24 x 150 = 9e-6 relative at the worst)
#   measured  on an MI355X: mfvit_cross_entropy loss 1.7e-7, dlogits 3.9e-6 (the floor: scale 30); mfvit_cross_entropy_soft loss 6.3e-7, dlogits
#             2.8e-7 (it scales exp(z - m) by 1 / s instead: no large lse in the exponent)
#   gates     at most 4 x the largest measured error, one significant digit
CE_SMALL_GATE = {"loss": 2e-6, "dlogits": 1e-5, "soft_loss": 2e-6, "soft_dlogits": 1e-6}


def log(msg):
    from test_ops_gpu import REPORT
    import os
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")


class Win:
    """`numel` elements at offset `off` inside a buffer filled with NaN (float32) or SENTINEL (int64); outside_intact() compares every word outside
    the window, intact() the whole buffer, with the state at construction."""

    def __init__(self, shape, dtype=torch.float32, off=1, value=None):
        numel = int(np.prod(shape))
        fill = NAN if dtype.is_floating_point else (SENTINEL if dtype == torch.int64 else SENTINEL >> 32)
        self.buf = torch.full((PAD + off + numel + PAD,), fill, device=DEV, dtype=dtype)
        self.lo, self.hi = PAD + off, PAD + off + numel
        self.view = self.buf[self.lo:self.hi].view(shape)
        if value is not None:
            self.view.copy_(value.to(DEV))
        self.before = self.buf.clone()
        self.ptr = self.view.data_ptr()

    def _bits(self, t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    def intact(self):
        return torch.equal(self._bits(self.buf), self._bits(self.before))

    def outside_intact(self):
        a, b = self._bits(self.buf), self._bits(self.before)
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.hi:], b[self.hi:])


def first_argmax(z):
    return torch.from_numpy(np.argmax(z.numpy(), axis=1))              # the first NaN, otherwise the first maximum: torch.max(z, 1)[1]


def f64_cross_entropy(z, t):
    zd = z.double().requires_grad_(True)
    rows = torch.nn.functional.cross_entropy(zd, t, reduction="none")
    rows.mean().backward()
    return float(rows.detach().mean()), zd.grad, float(rows.detach().max())


def run_hard(z, t, want_d=True, want_p=True):
    from mfvit._lib import check, lib, stream
    B, C = z.shape
    Z, T = Win((B, C), value=z, off=3), Win((B,), torch.int64, value=t)
    L, D, P = Win((1,), off=2), Win((B, C), off=1), Win((B,), torch.int64, off=1)
    check(lib().mfvit_cross_entropy(Z.ptr, T.ptr, L.ptr, D.ptr if want_d else None, P.ptr if want_p else None, B, C, stream()), "mfvit_cross_entropy")
    torch.cuda.synchronize()
    assert Z.intact() and T.intact() and L.outside_intact()
    assert D.outside_intact() if want_d else D.intact()
    assert P.outside_intact() if want_p else P.intact()
    return L.view.clone(), D.view.clone().cpu() if want_d else None, P.view.clone().cpu() if want_p else None


def run_soft(z, t, partner, lam, smoothing, want_d=True, want_p=True):
    from mfvit._lib import check, lib, stream
    B, C = z.shape
    Z, T = Win((B, C), value=z, off=3), Win((B,), torch.int64, value=t)
    Pa = La = None
    if partner is not None:
        Pa, La = Win((B,), torch.int32, value=partner, off=1), Win((B,), value=lam, off=2)
    L, D, P = Win((1,), off=2), Win((B, C), off=1), Win((B,), torch.int64, off=1)
    check(lib().mfvit_cross_entropy_soft(Z.ptr, T.ptr, Pa.ptr if Pa else None, La.ptr if La else None, smoothing, L.ptr, D.ptr if want_d else None,
                                         P.ptr if want_p else None, B, C, stream()), "mfvit_cross_entropy_soft")
    torch.cuda.synchronize()
    assert Z.intact() and T.intact() and L.outside_intact() and (Pa is None or (Pa.intact() and La.intact()))
    assert D.outside_intact() if want_d else D.intact()
    assert P.outside_intact() if want_p else P.intact()
    return L.view.clone(), D.view.clone().cpu() if want_d else None, P.view.clone().cpu() if want_p else None


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def errors(loss, d, ref_loss, ref_d, ref_rowmax, scale, B):
    over = ref_rowmax if scale > 1 else abs(ref_loss)
    e = dict(loss=abs(float(loss) - ref_loss) / max(over, 1e-30))
    if d is not None:
        e["dlogits"] = float((d.double() - ref_d).abs().max()) * B if not bool(torch.isnan(d).any()) else float("inf")
    return e


@pytest.mark.parametrize("C", ref_moco.CE_SMALL_C)
def test_cross_entropy_small_against_float64_at_every_trip_of_the_sample_loop(C):
    worst = dict(loss=0.0, dlogits=0.0, soft_loss=0.0, soft_dlogits=0.0)
    for B in ref_moco.CE_SMALL_B:
        for scale in ref_moco.CE_SMALL_SCALES:
            z, t = ref_moco.ce_small_case(B, C, scale)
            assert int(t.min()) >= 0 and int(t.max()) < C and int(t[-1]) == C - 1 and (B == 1 or int(t[0]) == 0)
            ref_loss, ref_d, ref_rowmax = f64_cross_entropy(z, t)
            want_p = first_argmax(z)
            if B > 1:
                assert int(want_p[1]) == C // 3                          # the tie row: the first of the two maxima
            loss, d, p = run_hard(z, t)
            e = errors(loss, d, ref_loss, ref_d, ref_rowmax, scale, B)
            assert torch.equal(p, want_p), (B, scale)
            loss2, d2, p2 = run_hard(z, t)
            assert same_bits(loss, loss2) and same_bits(d, d2) and torch.equal(p, p2), (B, scale)      # a fixed-order sum: the same bits
            loss3, d3, p3 = run_hard(z, t, want_d=False)
            loss4, d4, p4 = run_hard(z, t, want_p=False)
            assert d3 is None and p4 is None and same_bits(loss, loss3) and same_bits(loss, loss4) and torch.equal(p, p3) and same_bits(d, d4)
            # the soft kernel on the same hard targets (smoothing 0, no partner) against the same float64: both kernels in one place
            sl, sd, sp = run_soft(z, t, None, None, 0.0)
            es = errors(sl, sd, ref_loss, ref_d, ref_rowmax, scale, B)
            e.update(soft_loss=es["loss"], soft_dlogits=es["dlogits"])
            assert torch.equal(sp, want_p), (B, scale)
            for k, v in e.items():
                worst[k] = max(worst[k], v)
            assert all(v < CE_SMALL_GATE[k] for k, v in e.items()), (B, scale, e)
    log(f"cross_entropy small[C={C}, B in {list(ref_moco.CE_SMALL_B)}, scales {list(ref_moco.CE_SMALL_SCALES)}] " +
        " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  gates {CE_SMALL_GATE}")


@pytest.mark.parametrize("C", ref_moco.CE_SMALL_C)
def test_cross_entropy_soft_against_the_float64_oracle_at_every_trip_of_the_sample_loop(C):
    from test_mixup_gpu import ce_oracle
    worst = dict(loss=0.0, dlogits=0.0)
    for B in ref_moco.CE_SMALL_B:
        for scale in ref_moco.CE_SMALL_SCALES:
            z, t = ref_moco.ce_small_case(B, C, scale, seed=1)
            g = torch.Generator().manual_seed(B + C)
            perm, lam = torch.randperm(B, generator=g).int(), torch.rand(B, generator=g)
            lam[0], lam[-1] = 1.0, 0.0
            want_p = first_argmax(z)
            for partner, lm, smoothing in ((perm, lam, 0.1), (perm, lam, 0.0), (None, None, 0.1)):
                sm32 = float(np.float32(smoothing))
                ref_loss, ref_d = ce_oracle(z, t, partner, lm, sm32)
                # the largest row loss of this target, for the saturated measure: the oracle again, row by row, is the mean of B values; bound it by
                # the plain cross entropy's largest row (y is a convex mix of rows' one-hot and uniform targets: no row loss exceeds max_c -log p_c)
                rowmax = float((torch.logsumexp(z.double(), 1) - z.double().min(1).values).max())
                loss, d, p = run_soft(z, t, partner, lm, smoothing)
                e = errors(loss, d, ref_loss, ref_d, rowmax, scale, B)
                assert torch.equal(p, want_p), (B, scale, smoothing)
                loss2, d2, _ = run_soft(z, t, partner, lm, smoothing)
                assert same_bits(loss, loss2) and same_bits(d, d2), (B, scale, smoothing)
                loss3, d3, p3 = run_soft(z, t, partner, lm, smoothing, want_d=False, want_p=False)
                assert d3 is None and p3 is None and same_bits(loss, loss3)
                for k, v in e.items():
                    worst[k] = max(worst[k], v)
                assert all(v < CE_SMALL_GATE["soft_" + k] for k, v in e.items()), (B, scale, smoothing, partner is not None, e)
    log(f"cross_entropy_soft[C={C}, B in {list(ref_moco.CE_SMALL_B)}, scales {list(ref_moco.CE_SMALL_SCALES)}, partner / lam and smoothing on and off] " +
        " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  gates {CE_SMALL_GATE}")


def test_cross_entropy_rejects_more_than_64_classes_and_none_without_a_launch():
    from mfvit._lib import lib, stream
    for C in (65, 0):
        B = 4
        Z, T = Win((B, max(C, 1)), value=torch.zeros(B, max(C, 1))), Win((B,), torch.int64, value=torch.zeros(B, dtype=torch.int64))
        L, D, P = Win((1,)), Win((B, max(C, 1))), Win((B,), torch.int64)
        assert lib().mfvit_cross_entropy(Z.ptr, T.ptr, L.ptr, D.ptr, P.ptr, B, C, stream()) == EINVAL
        assert lib().mfvit_cross_entropy_soft(Z.ptr, T.ptr, None, None, 0.0, L.ptr, D.ptr, P.ptr, B, C, stream()) == EINVAL
        torch.cuda.synchronize()
        assert L.intact() and D.intact() and P.intact()                  # nothing was written: no launch


def test_first_maximum_with_nan_is_torch_max_in_both_cross_entropies():
    """include/mfvit.h, "First maximum": the first NaN of a row wins, otherwise the first of the largest values.  A NaN row makes the mean NaN (as
    torch's); the gradient rows of the other samples do not notice."""
    rows = torch.tensor([[1, NAN, 3], [NAN, 2, 1], [3, 1, NAN], [2, 5, 5], [NAN, NAN, 7]])
    g = torch.Generator().manual_seed(3)
    more = torch.randn(1100, 3, generator=g)
    clean = more.clone()
    more[torch.rand(1100, 3, generator=g) < 0.1] = NAN
    z = torch.cat([rows, more])
    t = torch.randint(0, 3, (len(z),), generator=g)
    want = z.max(1)[1]
    assert want[:5].tolist() == [1, 0, 2, 1, 0] and torch.equal(want, first_argmax(z))
    ok = ~torch.isnan(z).any(1)
    _, ref_d, _ = f64_cross_entropy(torch.cat([rows.nan_to_num(0.0), clean]), t)
    for name, (loss, d, p) in (("dlogits", run_hard(z, t)), ("soft_dlogits", run_soft(z, t, None, None, 0.0))):
        assert torch.equal(p, want), name
        assert bool(torch.isnan(loss).all()), name
        assert float((d[ok].double() - ref_d[ok]).abs().max()) * len(z) < CE_SMALL_GATE[name], name
