"""Single-kernel parity of csrc/lora.hip through the C ABI (mfvit_lora_merge, mfvit_lora_grad) against float64 on the same f32 inputs, inside
NaN-filled buffers (as tests/test_optim_kernels_gpu.py): every byte outside the stated outputs must keep its bits.

Gates (tests/lora_ref.py) are forward-error bounds of the evaluation orders include/mfvit.h states, elementwise; nothing is measured:
  merge  |got - ref| <= (r + 2) 2^-24 (|w| + |s| sum_j |b| |a|)
  grad   |got - ref| <= (terms + 2) 2^-24 |s| sum |products|,  terms = N for da, K for db  (any summation tree)"""
import numpy as np
import pytest
import torch

import lora_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
SHAPES = [(384, 384), (1536, 384), (384, 1536), (768, 768), (4, 4), (1, 8)]
RANKS = [1, 3, 8, 16, 64]
S = float(np.float32(16.0 / 3.0))       # the scale crosses the C ABI as a float: the rounded value is the input
EINVAL = -22


def lib():
    from mfvit import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A [rows][cols] f32 matrix with row stride ld inside a NaN-filled buffer, PAD NaNs around it; `mask` marks the matrix elements."""

    def __init__(self, values, ld=None):
        rows, cols = values.shape
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        n = (rows - 1) * self.ld + cols
        self.buf = torch.full((PAD + n + PAD,), float("nan"), device=DEV, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0 and PAD % 4 == 0
        idx = (torch.arange(rows)[:, None] * self.ld + torch.arange(cols)[None, :]).reshape(-1) + PAD
        self.idx = idx.to(DEV)
        self.buf[self.idx] = values.reshape(-1).to(DEV)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def row_ptr(self, r):
        return self.ptr + 4 * r * self.ld

    def get(self):
        return self.buf[self.idx].reshape(self.rows, self.cols).cpu()

    def outside_untouched(self, rows=None):
        """Everything but the matrix elements (of the given rows: default all) still has its bits."""
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        idx = self.idx.reshape(self.rows, self.cols)
        keep[(idx if rows is None else idx[rows]).reshape(-1)] = False
        return torch.equal(self.buf.view(torch.int32)[keep], self.before.view(torch.int32)[keep])


def inputs(N, K, r, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g)
    a = (torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5
    b = torch.randn(N, r, generator=g)
    return w, a, b


def merge(w, ldw, a, b, s, out, ldo, N, K, r):
    return lib().mfvit_lora_merge(w, ldw, a, b, s, out, ldo, N, K, r, stream())


def grad(dw, lddw, a, b, s, da, db, N, K, r):
    return lib().mfvit_lora_grad(dw, lddw, a, b, s, da, db, N, K, r, stream())


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_merge_matches_float64_within_its_error_bound(N, K, r):
    w, a, b = inputs(N, K, r, 100 + r)
    ref, gate = lora_ref.merge_ref_and_gate(w, a, b, S)
    A, B = Guarded(a), Guarded(b)
    worst = 0.0
    for ldw, ldo in ((K, K), (K + 4, K + 8)):
        W, O = Guarded(w, ldw), Guarded(torch.zeros(N, K), ldo)
        assert merge(W.ptr, ldw, A.ptr, B.ptr, S, O.ptr, ldo, N, K, r) == 0
        torch.cuda.synchronize()
        worst = max(worst, lora_ref.within(O.get(), ref, gate))
        assert O.outside_untouched() and torch.equal(W.buf.view(torch.int32), W.before.view(torch.int32))
    # in place (out == w), padded
    W = Guarded(w, K + 4)
    assert merge(W.ptr, K + 4, A.ptr, B.ptr, S, W.ptr, K + 4, N, K, r) == 0
    torch.cuda.synchronize()
    worst = max(worst, lora_ref.within(W.get(), ref, gate))
    assert W.outside_untouched()
    # the middle row block of a fused [3N][K] matrix (the k rows of attn.qkv.weight), in place: the q and v rows keep their bits
    wide = torch.cat([torch.randn(N, K), w, torch.randn(N, K)], dim=0)
    W3 = Guarded(wide)
    assert merge(W3.row_ptr(N), K, A.ptr, B.ptr, S, W3.row_ptr(N), K, N, K, r) == 0
    torch.cuda.synchronize()
    worst = max(worst, lora_ref.within(W3.get()[N:2 * N], ref, gate))
    assert W3.outside_untouched(rows=slice(N, 2 * N))
    assert torch.equal(A.buf.view(torch.int32), A.before.view(torch.int32)) and torch.equal(B.buf.view(torch.int32), B.before.view(torch.int32))
    print(f"merge N={N} K={K} r={r}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("r", [1, 8, 64])
@pytest.mark.parametrize("N,K", [(384, 384), (4, 4), (1, 8)])
def test_merge_with_zero_b_returns_the_bits_of_w(N, K, r):
    w, a, _ = inputs(N, K, r, 7)
    w.view(-1)[0] = -0.0
    w.view(-1)[1] = 1e-42                     # a subnormal
    a.view(-1)[0] = -3.0                      # (0 * negative = -0: still no change)
    W, O, A, B = Guarded(w), Guarded(torch.ones(N, K), K + 4), Guarded(a), Guarded(torch.zeros(N, r))
    assert merge(W.ptr, K, A.ptr, B.ptr, S, O.ptr, K + 4, N, K, r) == 0
    torch.cuda.synchronize()
    assert torch.equal(O.get().view(torch.int32), w.view(torch.int32))
    assert O.outside_untouched()


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_grad_matches_float64_is_reproducible_and_stays_inside_its_outputs(N, K, r):
    dw, a, b = inputs(N, K, r, 200 + r)
    (da_ref, ga), (db_ref, gb) = lora_ref.grad_ref_and_gate(dw, a, b, S)
    A, B = Guarded(a), Guarded(b)
    worst = [0.0, 0.0]
    bits = []
    for lddw in (K, K + 12, K):
        DW = Guarded(dw, lddw)
        DA, DB = Guarded(torch.full((r, K), 7.0)), Guarded(torch.full((N, r), -7.0))      # overwritten, not accumulated into
        assert grad(DW.ptr, lddw, A.ptr, B.ptr, S, DA.ptr, DB.ptr, N, K, r) == 0
        torch.cuda.synchronize()
        worst[0] = max(worst[0], lora_ref.within(DA.get(), da_ref, ga))
        worst[1] = max(worst[1], lora_ref.within(DB.get(), db_ref, gb))
        assert DA.outside_untouched() and DB.outside_untouched()
        assert torch.equal(DW.buf.view(torch.int32), DW.before.view(torch.int32))
        bits.append((DA.get().view(torch.int32), DB.get().view(torch.int32)))
    print(f"grad N={N} K={K} r={r}: worst error / bound da {worst[0]:.3f} db {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    for x, y in bits[1:]:                     # the same bits on every call, whatever the stride of dw
        assert torch.equal(x, bits[0][0]) and torch.equal(y, bits[0][1])


def test_domain_edges_return_einval_before_any_launch():
    N, K, r = 8, 8, 4
    w, a, b = inputs(N, K, 64, 3)
    W, A, B = Guarded(w, K + 4), Guarded(a), Guarded(b)
    O, DA, DB = Guarded(torch.zeros(N, K), K + 4), Guarded(torch.zeros(64, K)), Guarded(torch.zeros(N, 64))

    def m(**kw):
        p = dict(w=W.ptr, ldw=K + 4, a=A.ptr, b=B.ptr, s=S, out=O.ptr, ldo=K + 4, N=N, K=K, r=r)
        p.update(kw)
        return merge(p["w"], p["ldw"], p["a"], p["b"], p["s"], p["out"], p["ldo"], p["N"], p["K"], p["r"])

    def g(**kw):
        p = dict(dw=W.ptr, lddw=K + 4, a=A.ptr, b=B.ptr, s=S, da=DA.ptr, db=DB.ptr, N=N, K=K, r=r)
        p.update(kw)
        return grad(p["dw"], p["lddw"], p["a"], p["b"], p["s"], p["da"], p["db"], p["N"], p["K"], p["r"])

    # the valid side of every edge
    for f in (m, g):
        assert f() == 0
        assert f(r=1) == 0 and f(r=64) == 0
        assert f(K=4) == 0 and f(N=1) == 0
    dense = Guarded(torch.zeros(N, K))
    assert m(ldw=K, out=dense.ptr, ldo=K) == 0 and g(lddw=K) == 0        # a row stride equal to the row
    # the other side
    for f in (m, g):
        assert f(r=0) == EINVAL and f(r=65) == EINVAL and f(r=-1) == EINVAL
        assert f(K=6) == EINVAL and f(K=0) == EINVAL and f(K=2) == EINVAL
        assert f(N=0) == EINVAL
        assert f(a=None) == EINVAL and f(b=None) == EINVAL
        assert f(a=A.ptr + 4) == EINVAL                                   # 16-byte accesses along k
    assert m(w=None) == EINVAL and m(out=None) == EINVAL
    assert m(ldw=K - 4) == EINVAL and m(ldo=K - 4) == EINVAL              # a row stride smaller than the row
    assert m(ldw=K + 2) == EINVAL and m(ldo=K + 1) == EINVAL              # ... or off the 16-byte grid
    assert m(w=W.ptr + 4) == EINVAL and m(out=O.ptr + 8) == EINVAL
    assert g(dw=None) == EINVAL and g(da=None) == EINVAL and g(db=None) == EINVAL
    assert g(lddw=K - 4) == EINVAL and g(lddw=K + 3) == EINVAL
    assert g(dw=W.ptr + 4) == EINVAL and g(da=DA.ptr + 12) == EINVAL
    torch.cuda.synchronize()
    assert O.outside_untouched() and DA.outside_untouched() and DB.outside_untouched()
