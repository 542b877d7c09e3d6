"""The five BatchNorm entry points of the MoCo projector / predictor (mfvit_bn_stats / _combine / _apply / _bwd_sums / _bwd_apply, csrc/moco.hip),
each on its own through the C ABI against its float64 statement in oracle/ref_moco.py on the same rounded inputs, at the shapes where their
address arithmetic can go wrong (tests/test_bn_gpu.py runs them through HipBatchNorm1d at n in {32, 128}, C in {256, 512, 4096}, aligned):
  both kernels of each dispatch   mfvit_bn_stats and mfvit_bn_bwd_sums take the tiled kernels (16 row groups x 16 column quads, 64 columns per
                      workgroup) when C % 4 == 0 and every pointer is 16-byte aligned, the column-per-thread kernels otherwise: C % 4 != 0 (C = 257
                      crosses their 256-thread block), x off by one element (and by four elements, 8 bytes, in the 16-bit types), dy, x, y off one
                      at a time.  Which kernel a call takes is worked out here from the pointers, and both must have run for every type.
  tile edges          one quad (C = 4), a partial 64-column block (60), a second block with a single live quad (68), several blocks (256, 260, 1028);
                      n below, at and one past the 16 row groups, and a third sweep with one live group (33)
  options             relu 0 / 1, gamma NULL / given, running statistics NULL / given
  the ReLU mask       y is an input of the backward: positive values, +0.0, -0.0, negative values and NaN by hand; all but the first are masked
  values              an exactly constant column (M2 == 0, invstd = rsqrt(eps), y == beta, dx finite), a column with mean >> std, n = 1
  mfvit_bn_combine    W = 1, ragged W = 3, W = 8 with an empty rank first, in the middle and last (finite garbage in its mean and M2)
Every buffer is a view inside a larger NaN-filled tensor: the bytes outside the documented windows are compared bit for bit, the inputs too.
Measured errors go to parity_bn.txt beside those of tests/test_bn_gpu.py; tests/test_step_refs_cpu.py pins the references and prints the floors."""
import numpy as np
import pytest
import torch

from oracle import ref_moco

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                  # guard elements before and behind every view: 128 bytes in the 16-bit types, so the view's 16-byte phase is its offset
NAN = float("nan")
EPS32, MOM32 = float(np.float32(1e-5)), float(np.float32(0.1))          # the floats the kernels receive

# Gates: max abs error over the reference's max abs per output (rel() of tests/test_bn_gpu.py), against float64 on the same inputs.  Set by the recipe
# above CE_GATE in tests/test_moco_rowops_gpu.py: floor on the CPU (tests/test_step_refs_cpu.py prints it), measured on an MI355X over the whole
# matrix, gate at most 4 x the largest measured error at one significant digit, never above the project's ceiling.
#   STAT_GATE     mean, m2, invstd, s1, s2, running statistics (float32 in every element type).  ceiling 5e-5
#                 floor     float32 two-pass restatement over the whole matrix: 5.1e-7 (f32), 2.4e-7 (fp16), 3.3e-7 (bf16); the mean >> std column on
#                           its own scale 2.2e-7 / 2.1e-7 / 1.7e-7 (a one-pass variance there: 4.5e-3 and more in f32)
#                 measured  mean 5.1e-7, m2 3.3e-7, invstd 8.2e-8, running mean / var 9.4e-8 / 9.0e-8, s1 7.3e-7, s2 1.7e-6 (a sum of at most 33
#                           products of either sign: small n and C, where every column's sum is small beside its terms)
#   COMBINE_GATE  mfvit_bn_combine on float32 triples.  ceiling 2e-5 (test_chan_combine_of_eight_partial_statistics)
#                 floor     float32 restatement of the rank-by-rank update: 1.6e-7
#                 measured  mean 1.6e-7, invstd 1.1e-7, running mean / var 9.3e-8 / 1.3e-7 - the floor itself: the gate is 4 x that
#   OUT_GATE      y and dx, which leave the kernels in the element type: one rounding of the result (at most 2^-24 f32, 2^-11 = 4.9e-4 fp16,
#                 2^-8 = 3.9e-3 bf16 of the tensor's max abs) on top of float32 arithmetic.  ceilings: TOL of tests/test_bn_gpu.py
#                 floor     the float64 y rounded to the element type 5.2e-8 / 4.5e-4 / 3.8e-3; dx in float32 before that rounding 1.5e-7
#                 measured  y 1.1e-7 / 4.6e-4 / 3.8e-3, dx 1.8e-7 / 4.6e-4 / 3.6e-3
#                 dx at n = 2 vanishes identically (xhat = +-1 up to eps / var): 1e-2 of its own size in the float32 restatement alone, 2.5e-8 of its
#                 terms.  There, and only there, the error is taken over ref_moco.bn_bwd_apply_terms() instead of the result's max abs.
STAT_GATE = 5e-6
COMBINE_GATE = 6e-7
OUT_GATE = {"f32": 7e-7, "fp16": 1e-3, "bf16": 1e-2}


def log(msg):
    from test_bn_gpu import log as bn_log                          # parity_bn.txt
    bn_log(msg)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    if bool(torch.isnan(a).any()):
        return float("inf")
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Guarded:
    """`shape` elements of `dtype` at element offset `off` inside a NaN-filled buffer; `untouched(writable)` compares every byte outside the view
    (writable=True) or the whole buffer (writable=False) with what it held when snap() was called."""

    def __init__(self, shape, dtype=torch.float32, off=0, value=None):
        numel = int(np.prod(shape))
        self.buf = torch.full((PAD + off + numel + PAD,), NAN, device=DEV, dtype=dtype)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = PAD + off, PAD + off + numel
        self.view = self.buf[self.lo:self.hi].view(shape)
        if value is not None:
            self.view.copy_(value.to(DEV))
        self.snap()

    def snap(self):
        self.before = self.buf.clone()

    def untouched(self, writable):
        bits = torch.int32 if self.buf.dtype == torch.float32 else torch.int16
        a, b = self.buf.view(bits), self.before.view(bits)
        if not writable:
            return torch.equal(a, b)
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.hi:], b[self.hi:])

    @property
    def ptr(self):
        return self.view.data_ptr()


def all_untouched(inputs, outputs):
    return all(g.untouched(False) for g in inputs) and all(g.untouched(True) for g in outputs)


def code_of(dtype):
    from mfvit import ops
    return ops._code_of_dtype(dtype)


def misalignments(prec):
    """element offsets of a view: aligned, one element off, and (16-bit types) four elements = 8 bytes off, where a quad load would still be aligned"""
    return (0, 1) if prec == "f32" else (0, 1, 4)


# ------------------------------------------------------------------------------------------------ the four per-element-type entry points
@pytest.mark.parametrize("C", ref_moco.BN_C)
@pytest.mark.parametrize("prec", list(ref_moco.BN_DTYPES))
def test_bn_entry_points_on_both_kernels_of_each_dispatch(prec, C):
    from mfvit._lib import check, lib, stream
    dt, code = ref_moco.BN_DTYPES[prec], code_of(ref_moco.BN_DTYPES[prec])
    worst = {k: 0.0 for k in ("mean", "m2", "invstd", "run_mean", "run_var", "y", "s1", "s2", "dx")}
    stats_tiled, sums_tiled, cases = set(), set(), 0
    rsqrt_eps = 1.0 / np.sqrt(np.float32(EPS32), dtype=np.float32)

    def gate_of(k):
        return OUT_GATE[prec] if k in ("y", "dx") else STAT_GATE

    def judge(e, what):
        for k, v in e.items():
            worst[k] = max(worst[k], v)
        assert all(v < gate_of(k) for k, v in e.items()), (what, e)

    for n in ref_moco.BN_N:
        for family in ("plain", "edge"):
            x, dy, y_hand, gamma, beta = (t.to(DEV) for t in ref_moco.bn_case_inputs(prec, n, C, family))
            gm, bt = Guarded((C,), off=1, value=gamma), Guarded((C,), off=2, value=beta)
            options = [(r, a) for r in (0, 1) for a in (0, 1)] if family == "plain" else [(1, 1)]
            # ---- mfvit_bn_stats at every alignment of x, then mfvit_bn_combine of the one triple (running statistics given for odd n, NULL for even)
            for xoff in misalignments(prec):
                X = Guarded((n, C), dt, xoff, x)
                tiled = C % 4 == 0 and X.ptr % 16 == 0
                assert X.ptr % 16 == (xoff * x.element_size()) % 16
                stats_tiled.add(tiled)
                mean_k, m2_k = Guarded((C,), off=3), Guarded((C,), off=1)
                check(lib().mfvit_bn_stats(code, X.ptr, n, C, mean_k.ptr, m2_k.ptr, stream()), "mfvit_bn_stats")
                torch.cuda.synchronize()
                assert all_untouched([X], [mean_k, m2_k]), (n, family, xoff)
                r_mean, r_m2 = ref_moco.bn_stats(X.view)
                what = (n, family, "stats", "tiled" if tiled else "column", xoff)
                judge(dict(mean=rel(mean_k.view, r_mean), m2=rel(m2_k.view, r_m2)), what)
                if family == "edge" or n == 1:
                    cols = slice(0, 1) if n > 1 else slice(0, C)                          # the constant column; with one row every column is constant
                    assert not bool(m2_k.view[cols].any()), what                           # M2 is exactly 0
                    assert torch.equal(mean_k.view[cols], X.view[0, cols].float()), what   # and the mean the value itself
                    if C > 1 and n > 1:                                                    # mean >> std: measured on the column's own scale
                        e_m, e_q = float((mean_k.view[1] - r_mean[1]).abs() / r_mean[1].abs()), float((m2_k.view[1] - r_m2[1]).abs() / r_m2[1].clamp_min(1e-30))
                        worst["mean"], worst["m2"] = max(worst["mean"], e_m), max(worst["m2"], e_q)
                        assert e_m < STAT_GATE and e_q < STAT_GATE, (what, e_m, e_q)
            cnt = Guarded((1,), off=1, value=torch.tensor([float(n)]))
            mean, invstd = Guarded((C,), off=2), Guarded((C,), off=3)
            run = n % 2 == 1
            mean_k.snap(), m2_k.snap()
            rm, rv = Guarded((C,), off=1, value=0.3 * beta), Guarded((C,), off=3, value=gamma)
            check(lib().mfvit_bn_combine(mean_k.ptr, m2_k.ptr, cnt.ptr, 1, C, EPS32, MOM32, mean.ptr, invstd.ptr, rm.ptr if run else None,
                                         rv.ptr if run else None, stream()), "mfvit_bn_combine")
            torch.cuda.synchronize()
            assert all_untouched([mean_k, m2_k, cnt] + ([] if run else [rm, rv]), [mean, invstd] + ([rm, rv] if run else [])), (n, family)
            r_mu, r_is, r_rm, r_rv = ref_moco.bn_combine(mean_k.view[None], m2_k.view[None], cnt.view, EPS32, MOM32, rm.before[rm.lo:rm.hi],
                                                         rv.before[rv.lo:rv.hi])
            e = dict(mean=rel(mean.view, r_mu), invstd=rel(invstd.view, r_is))
            if run:
                e.update(run_mean=rel(rm.view, r_rm), run_var=rel(rv.view, r_rv))
            judge(e, (n, family, "combine"))
            if family == "edge" or n == 1:
                cols = slice(0, 1) if n > 1 else slice(0, C)
                # invstd of a constant column is rsqrtf(0 + eps): within 2 ulp of the rounded 1 / sqrt(eps) (the device rsqrt is good to 1 ulp)
                assert float((invstd.view[cols].double() - float(rsqrt_eps)).abs().max()) <= 2.0 ** -22 * float(rsqrt_eps), (n, family)
            if n == 1 and run:                                                             # the `N > 1.f ? ... : var` branch: the biased value, 0
                assert rel(rv.view, (1.0 - MOM32) * rv.before[rv.lo:rv.hi].double()) < STAT_GATE
            mean.snap(), invstd.snap()
            for relu, affine in options:
                g_ptr, b_ptr = (gm.ptr, bt.ptr) if affine else (None, None)
                what = (n, family, f"relu={relu}", f"affine={affine}")
                cases += 1
                # ---- mfvit_bn_apply
                X, Y = Guarded((n, C), dt, 1, x), Guarded((n, C), dt, 3)
                check(lib().mfvit_bn_apply(code, X.ptr, mean.ptr, invstd.ptr, g_ptr, b_ptr, relu, Y.ptr, n, C, stream()), "mfvit_bn_apply")
                torch.cuda.synchronize()
                assert all_untouched([X, mean, invstd, gm, bt], [Y]), what
                r_y = ref_moco.bn_apply(X.view, mean.view, invstd.view, gm.view if affine else None, bt.view if affine else None, relu)
                judge(dict(y=rel(Y.view, r_y)), what + ("apply",))
                if family == "edge" or n == 1:                                             # y of a constant column is beta itself (0 without affine)
                    cols = slice(0, 1) if n > 1 else slice(0, C)
                    want = (bt.view[cols] if affine else torch.zeros_like(bt.view[cols])).clamp_min(0.0 if relu else -1e30).to(dt)
                    assert torch.equal(Y.view[:, cols], want.expand(n, -1)), what
                # ---- mfvit_bn_bwd_sums with dy, x, y off one at a time; y: hand-built with relu, NULL or NaN-filled without
                pass_y = bool(relu) or n % 2 == 0                                          # without relu y is not read: NULL, or NaN in every element
                for which in ("none", "dy", "x", "y"):
                    for off in misalignments(prec)[1:] if which != "none" else (0,):
                        offs = {k: (off if k == which else 0) for k in ("dy", "x", "y")}
                        G, X = Guarded((n, C), dt, offs["dy"], dy), Guarded((n, C), dt, offs["x"], x)
                        Yh = Guarded((n, C), dt, offs["y"], y_hand if relu else None)
                        tiled = C % 4 == 0 and G.ptr % 16 == 0 and X.ptr % 16 == 0 and (not relu or Yh.ptr % 16 == 0)
                        sums_tiled.add(tiled)
                        s1, s2 = Guarded((C,), off=1), Guarded((C,), off=2)
                        check(lib().mfvit_bn_bwd_sums(code, G.ptr, X.ptr, Yh.ptr if pass_y else None, mean.ptr, invstd.ptr, relu, n, C, s1.ptr, s2.ptr,
                                                      stream()), "mfvit_bn_bwd_sums")
                        torch.cuda.synchronize()
                        assert all_untouched([G, X, Yh, mean, invstd], [s1, s2]), (what, which, off)
                        r_s1, r_s2 = ref_moco.bn_bwd_sums(G.view, X.view, Yh.view, mean.view, invstd.view, relu)
                        judge(dict(s1=rel(s1.view, r_s1), s2=rel(s2.view, r_s2)), what + ("bwd_sums", "tiled" if tiled else "column", which, off))
                # ---- mfvit_bn_bwd_apply on the sums of the last call
                G, X, Yh = Guarded((n, C), dt, 1, dy), Guarded((n, C), dt, 0, x), Guarded((n, C), dt, 3, y_hand if relu else None)
                DX = Guarded((n, C), dt, 1)
                s1.snap(), s2.snap()
                inv_count = float(np.float32(1.0 / n))
                check(lib().mfvit_bn_bwd_apply(code, G.ptr, X.ptr, Yh.ptr if pass_y else None, mean.ptr, invstd.ptr, g_ptr, relu, s1.ptr, s2.ptr, inv_count,
                                               DX.ptr, n, C, stream()), "mfvit_bn_bwd_apply")
                torch.cuda.synchronize()
                assert all_untouched([G, X, Yh, mean, invstd, gm, s1, s2], [DX]), what
                r_dx = ref_moco.bn_bwd_apply(G.view, X.view, Yh.view, mean.view, invstd.view, gm.view if affine else None, relu, s1.view, s2.view, inv_count)
                assert bool(torch.isfinite(DX.view).all()), what                           # the constant column and n = 1 included
                if n == 2:             # dx vanishes identically (ref_moco.bn_bwd_apply_terms): held to the scale of its terms, not to its own
                    terms = ref_moco.bn_bwd_apply_terms(G.view, X.view, Yh.view, mean.view, invstd.view, gm.view if affine else None, relu, s1.view, s2.view,
                                                        inv_count)
                    judge(dict(dx=float((DX.view.double() - r_dx).abs().max()) / max(terms, 1e-30)), what + ("bwd_apply", "terms"))
                else:
                    judge(dict(dx=rel(DX.view, r_dx)), what + ("bwd_apply",))
    log(f"bn entry points[{prec}, C={C}, {cases} option cases x n in {list(ref_moco.BN_N)}] " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
        f"  gates: statistics {STAT_GATE:.0e}, y / dx {OUT_GATE[prec]:.0e}")
    # coverage, from the pointer arithmetic above: both kernels of each dispatch ran for this type wherever the tiled one can run at all
    want = {True, False} if C % 4 == 0 else {False}
    assert stats_tiled == want and sums_tiled == want, (stats_tiled, sums_tiled)


def test_bn_case_matrix_reaches_both_kernels_in_every_type():
    """the coverage statement of the matrix as a whole: tiled-capable widths (C % 4 == 0) and column-only widths are both in it, in every type"""
    assert {c % 4 == 0 for c in ref_moco.BN_C} == {True, False}
    assert set(ref_moco.BN_DTYPES) == {"f32", "fp16", "bf16"} and all(1 in misalignments(p) for p in ref_moco.BN_DTYPES)


# ------------------------------------------------------------------------------------------------ mfvit_bn_combine
GARBAGE_MEAN, GARBAGE_M2 = 1e30, 7.0                                    # what an empty rank may hold: finite, and fatal if it is used


@pytest.mark.parametrize("C", [1, 5, 256, 257, 1028])
def test_bn_combine_ragged_counts_and_empty_ranks(C):
    from mfvit._lib import check, lib, stream
    worst = {}

    def run(means, m2s, counts, eps, mom, running):
        W = len(counts)
        M, Q, K = Guarded((W, C), off=1, value=means), Guarded((W, C), off=2, value=m2s), Guarded((W,), off=3, value=counts)
        mean, invstd = Guarded((C,), off=1), Guarded((C,), off=2)
        g = torch.Generator().manual_seed(C)
        rm, rv = Guarded((C,), off=3, value=torch.randn(C, generator=g)), Guarded((C,), off=1, value=0.5 + torch.rand(C, generator=g))
        check(lib().mfvit_bn_combine(M.ptr, Q.ptr, K.ptr, W, C, eps, mom, mean.ptr, invstd.ptr, rm.ptr if running else None, rv.ptr if running else None,
                                     stream()), "mfvit_bn_combine")
        torch.cuda.synchronize()
        assert all_untouched([M, Q, K] + ([] if running else [rm, rv]), [mean, invstd] + ([rm, rv] if running else []))
        r = ref_moco.bn_combine(M.view, Q.view, K.view, eps, mom, rm.before[rm.lo:rm.hi], rv.before[rv.lo:rv.hi])
        got = [mean.view.clone(), invstd.view.clone()] + ([rm.view.clone(), rv.view.clone()] if running else [])
        e = {k: rel(a, b) for k, a, b in zip(("mean", "invstd", "run_mean", "run_var"), got, r)}
        return got, e

    for name, counts in ref_moco.BN_COMBINE_COUNTS.items():
        means, m2s, cnt = ref_moco.bn_combine_inputs(C, counts)
        for eps, mom in ((EPS32, MOM32), (float(np.float32(1e-3)), float(np.float32(0.37)))):
            for running in (False, True):
                full, e = run(means, m2s, cnt, eps, mom, running)
                for k, v in e.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                assert all(v < COMBINE_GATE for v in e.values()), (name, eps, mom, e)
            if len(counts) != 8:
                continue
            # an empty rank first, in the middle, last: the result of the seven others, bit for bit (the same additions in the same order), as
            # torch's SyncBatchNorm leaves a rank with count 0 out - and within the gate of float64
            for pos in (0, 4, 8):
                m9 = torch.cat([means[:pos], torch.full((1, C), GARBAGE_MEAN), means[pos:]])
                q9 = torch.cat([m2s[:pos], torch.full((1, C), GARBAGE_M2), m2s[pos:]])
                k9 = torch.cat([cnt[:pos], torch.zeros(1), cnt[pos:]])
                got, e = run(m9, q9, k9, eps, mom, True)
                assert all(v < COMBINE_GATE for v in e.values()), (name, "empty rank at", pos, e)
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, full)), (name, "empty rank at", pos)
    log(f"bn_combine[C={C}, {list(ref_moco.BN_COMBINE_COUNTS)}, empty rank at 0 / 4 / 8, eps and momentum default and (1e-3, 0.37)] " +
        " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  gate {COMBINE_GATE:.0e}")
