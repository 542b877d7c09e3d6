"""GPU tests of attention-guided token pruning between blocks: the kernels of csrc/token_prune.hip and the block-range entry points
(mfvit_vit_forward_seg / _backward_seg) through the C ABI, then the model path (vits.vit_small(token_keep_rate=..), Fus_CrossViT) against the
float64 restatement tests/token_prune_ref.py on the inputs that file fixes.  Gates of the model tests: patch_drop_ref.CAPS, the ones the
unpruned encoder meets.  Every test of this file fails on a tree without the feature: neither the constructor arguments nor the symbols exist."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import token_prune_ref as R
from fusion_edges_ref import GATES as FUSION_GATES
from mfvit import _lib
from mfvit._lib import MfvitError, check, lib, ptr, stream
from oracle import ref_fusion, ref_vit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["fp32", "bf16x3", "bf16", "fp16"]
EPS = 2.0 ** -24                                    # unit roundoff of f32
FUS_MOD = ("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
           "changemodelinputlocation_std002_sum")
NAN = float("nan")


def guarded(shape, dtype, guard=64):
    """A device tensor of `shape` inside a NaN (float) / -7777 (int) band of `guard` elements on either side: (whole buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), NAN if dtype.is_floating_point else -7777, device=DEV, dtype=dtype)
    return buf, buf[guard:guard + n].view(shape)


def band_untouched(buf, n, guard=64):
    band = torch.cat([buf[:guard], buf[guard + n:]])
    return bool(torch.isnan(band).all()) if buf.dtype.is_floating_point else bool((band == -7777).all())


def select_gpu(score, K, forced=None):
    B, P = score.shape
    s = score.to(DEV).contiguous()
    bk, ik = guarded((B, K), torch.int32)
    bd, idr = guarded((B, P - K), torch.int32)
    bw, w = guarded((B, P - K), torch.float32)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    f = None if forced is None else forced.to(DEV, torch.int32).contiguous()
    check(lib().mfvit_token_select(ptr(s), P, B, P, K, ptr(f), ptr(ik), ptr(idr) if P > K else None, ptr(w) if P > K else None, ptr(err),
                                   stream()), "mfvit_token_select")
    torch.cuda.synchronize()
    assert band_untouched(bk, B * K) and band_untouched(bd, B * (P - K)) and band_untouched(bw, B * (P - K))
    return ik.cpu().numpy(), idr.cpu().numpy(), w.cpu().numpy(), int(err.item())


def reorg_fwd_gpu(x, keep, drop, w, fuse, err=None):
    B, T, D = x.shape
    K = keep.shape[1]
    bo, out = guarded((B, 1 + K + fuse, D), torch.float32)
    err = torch.zeros(1, device=DEV, dtype=torch.int32) if err is None else err
    check(lib().mfvit_token_reorg_fwd(ptr(x), ptr(keep), ptr(drop), ptr(w), ptr(out), B, T, D, K, fuse, ptr(err), stream()), "mfvit_token_reorg_fwd")
    torch.cuda.synchronize()
    assert band_untouched(bo, out.numel())
    return out, int(err.item())


def reorg_bwd_gpu(dout, keep, drop, w, T, fuse):
    B, _, D = dout.shape
    K = keep.shape[1]
    bx, dx = guarded((B, T, D), torch.float32)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    check(lib().mfvit_token_reorg_bwd(ptr(dout), ptr(keep), ptr(drop), ptr(w), ptr(dx), B, T, D, K, fuse, ptr(err), stream()), "mfvit_token_reorg_bwd")
    torch.cuda.synchronize()
    assert band_untouched(bx, dx.numel())
    return dx, int(err.item())


def ks_of(T):
    return sorted({1, max(1, (T - 1) // 2), max(1, T - 2)})


# --------------------------------------------------------------------------------------------------- kernels through the C ABI
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [3, 4, 37, 129, 197])
def test_select_matches_the_reference_to_the_bit(B, T):
    """Index lists: exact integers.  Weights: the reference repeats the kernel's arithmetic (the dropped scores added in ascending order in f32,
    one IEEE f32 division each), so w is compared bit for bit."""
    P = T - 1
    score = torch.from_numpy(np.random.Generator(np.random.PCG64(700 + 10 * T + B)).random((B, P), dtype=np.float32))
    for K in ks_of(T):
        if K >= P:
            continue
        keep, drop, w, err = select_gpu(score, K)
        rk, rd, rw = R.select_ref(score.numpy(), K)
        assert err == 0 and np.array_equal(keep, rk) and np.array_equal(drop, rd), (T, K)
        assert np.array_equal(w.view(np.uint32), rw.view(np.uint32)), (T, K, np.abs(w - rw).max())
        keep2, drop2, w2, _ = select_gpu(score, K)
        assert np.array_equal(keep, keep2) and np.array_equal(drop, drop2) and np.array_equal(w.view(np.uint32), w2.view(np.uint32))


def test_select_special_scores():
    P, K = 12, 5
    s = torch.zeros(4, P)
    s[0] = torch.tensor([3, 1, 3, 3, 0, 1, 3, 2, 2, 3, 1, 0.0])                  # ties: the lower index wins
    s[1] = torch.tensor([NAN, 1, 2, NAN, 3, 4, NAN, NAN, NAN, NAN, NAN, NAN])    # NaN last; four numbers, so one NaN is kept - the lowest index
    s[2] = 0.0                                                                    # all zero: indices 0 .. K-1 kept, uniform weights
    s[3] = torch.tensor([5, 4, 3, 2, 1, 0, 0, 0, 0, 0, 0, 0.0])                  # the dropped sum is zero: uniform fallback
    keep, drop, w, err = select_gpu(s, K)
    rk, rd, rw = R.select_ref(s.numpy(), K)
    assert err == 0 and np.array_equal(keep, rk) and np.array_equal(drop, rd)
    assert keep[0].tolist() == [0, 2, 3, 6, 9] and keep[2].tolist() == [0, 1, 2, 3, 4]
    assert keep[1].tolist() == [0, 1, 2, 4, 5]
    u = np.float32(1.0) / np.float32(P - K)
    assert (w[1] == u).all() and (w[2] == u).all() and (w[3] == u).all()          # NaN sum, zero sum, zero sum
    assert np.array_equal(w[0].view(np.uint32), rw[0].view(np.uint32))
    # a single dropped row: its weight is exactly 1
    keep, drop, w, _ = select_gpu(s[:1], P - 1)
    assert w.tolist() == [[1.0]] and drop.tolist() == [[11]]
    # K == P: nothing is dropped
    keep, _, _, _ = select_gpu(s[:1], P)
    assert keep.tolist() == [list(range(P))]


def test_select_forced_reproduces_a_recorded_selection():
    B, P, K = 3, 36, 18
    score = torch.from_numpy(np.random.Generator(np.random.PCG64(811)).random((B, P), dtype=np.float32))
    keep, drop, w, _ = select_gpu(score, K)
    perm = torch.from_numpy(keep)[:, torch.randperm(K, generator=torch.Generator().manual_seed(1))]
    k2, d2, w2, err = select_gpu(score, K, forced=perm)
    assert err == 0 and np.array_equal(k2, keep) and np.array_equal(d2, drop) and np.array_equal(w2.view(np.uint32), w.view(np.uint32))
    other = torch.stack([torch.randperm(P, generator=torch.Generator().manual_seed(b))[:K] for b in range(B)])
    k3, d3, w3, err = select_gpu(score, K, forced=other)
    assert err == 0 and np.array_equal(k3, other.sort(dim=1)[0].numpy())
    # a list with an index out of range, or one named twice, keeps K - 1 rows: the error word, the tail of idx_keep at -1, the other images whole
    for b, bad in ((1, other.clone()), (2, other.clone())):
        if b == 1:
            bad[1, 2] = P
        else:
            bad[2, 3] = bad[2, 4]
        kb, _, _, err = select_gpu(score, K, forced=bad)
        good = sorted(set(v for v in bad[b].tolist() if v < P))
        assert err == 1 and len(good) == K - 1 and kb[b].tolist() == good + [-1]
        assert all(np.array_equal(kb[i], k3[i]) for i in range(B) if i != b)


@pytest.mark.parametrize("D", [384, 768])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [3, 4, 37, 129, 197])
def test_reorg_forward_and_backward(B, T, D):
    """Kept rows and every moved row of dx: bit for bit.  Dropped rows of dx: one f32 product, bit for bit.  The fused row: the kernel adds n
    terms t_j = w_j x_j per column as a = t_0 (rounded), a = fma(w_j, x_j, a): n roundings, each relative 2^-24 of a partial sum bounded by
    S = sum |t_j|, so |fused - exact| <= n 2^-24 S (Higham, Accuracy and Stability, eq. 4.4 with one rounding per term); the gate is
    twice that per column, against the float64 value of the same f32 inputs."""
    P = T - 1
    g = np.random.Generator(np.random.PCG64(900 + T + D + B))
    x = torch.from_numpy(g.standard_normal((B, T, D), dtype=np.float32)).to(DEV)
    score = torch.from_numpy(g.random((B, P), dtype=np.float32))
    for K in ks_of(T):
        if K >= P:
            continue
        keep, drop, w = R.select_ref(score.numpy(), K)
        ik, idr, wd = (torch.from_numpy(keep).to(DEV, torch.int32), torch.from_numpy(drop).to(DEV, torch.int32), torch.from_numpy(w).to(DEV))
        for fuse in (1, 0):
            out, err = reorg_fwd_gpu(x, ik, idr, wd, fuse)
            assert err == 0
            ref = R.reorg_fwd_ref(x.cpu().numpy(), keep, drop, w, fuse)
            o = out.cpu().numpy()
            assert np.array_equal(o[:, :1 + K].view(np.uint32), ref[:, :1 + K].astype(np.float32).view(np.uint32)), (T, K, fuse)
            if fuse:
                bound = 2.0 * (P - K) * EPS * R.reorg_fwd_abs(x.cpu().numpy(), drop, w) + 1e-45
                e = np.abs(o[:, 1 + K].astype(np.float64) - ref[:, 1 + K])
                assert (e <= bound).all(), (T, K, float((e / bound).max()))
                if P - K == 1:
                    assert np.array_equal(o[:, 1 + K].view(np.uint32), x.cpu().numpy()[np.arange(B), 1 + drop[:, 0]].view(np.uint32))
            out2, _ = reorg_fwd_gpu(x, ik, idr, wd, fuse)
            assert torch.equal(out, out2)
            dout = torch.from_numpy(g.standard_normal((B, 1 + K + fuse, D), dtype=np.float32)).to(DEV)
            dx, err = reorg_bwd_gpu(dout, ik, idr, wd, T, fuse)
            assert err == 0
            rdx = R.reorg_bwd_ref(dout.cpu().numpy(), keep, drop, w, T, fuse)
            assert np.array_equal(dx.cpu().numpy().view(np.uint32), rdx.view(np.uint32)), (T, K, fuse)
            dx2, _ = reorg_bwd_gpu(dout, ik, idr, wd, T, fuse)
            assert torch.equal(dx, dx2)


def test_reorg_bad_indices_set_the_error_word_and_write_zeros():
    B, T, D, K = 2, 9, 384, 3
    x = R.rng(951, (B, T, D)).to(DEV)
    keep = torch.tensor([[0, 2, 5], [1, 8, 6]], dtype=torch.int32, device=DEV)          # 8 == T - 1: outside [0, T - 1)
    drop = torch.tensor([[1, 3, 4, 6, 7], [0, 2, 3, 4, -1]], dtype=torch.int32, device=DEV)
    w = torch.full((B, 5), 0.2, device=DEV)
    out, err = reorg_fwd_gpu(x, keep, drop, w, 1)
    assert err == 1
    assert bool((out[1, 2] == 0).all()) and torch.equal(out[1, 1], x[1, 2]) and torch.equal(out[0, 1:4], x[0, [1, 3, 6]])
    ref = (0.2 * x[1, [1, 3, 4, 5]].double()).sum(0)
    assert float((out[1, 4].double() - ref).abs().max()) < 1e-5                         # the bad dropped index adds nothing
    dout = R.rng(952, (B, 1 + K + 1, D)).to(DEV)
    dx, err = reorg_bwd_gpu(dout, keep, drop, w, T, 1)
    assert err == 1 and torch.isfinite(dx).all()
    assert bool((dx[1, 1 + 7] == 0).all()) and bool((dx[1, 1 + 5] == 0).all())         # rows no valid entry names
    assert torch.equal(dx[1, 1 + 6], dout[1, 3]) and torch.equal(dx[0, 0], dout[0, 0])
    # a repeated index: the error word
    keep2 = torch.tensor([[0, 2, 2], [1, 5, 6]], dtype=torch.int32, device=DEV)
    drop2 = torch.tensor([[1, 3, 4, 6, 7], [0, 2, 3, 4, 7]], dtype=torch.int32, device=DEV)
    assert reorg_fwd_gpu(x, keep2, drop2, w, 1)[1] == 1
    assert reorg_bwd_gpu(dout, keep2, drop2, w, T, 1)[1] == 1


def build(c, precision, **kw):
    import vits
    m = getattr(vits, R.arch_of(c))(num_classes=3, depth=c["depth"], precision=precision, img_size=c["hw"], num_heads=c["heads"], **kw)
    m.load_state_dict(R.case_params(c), strict=True)
    return m.to(DEV)


def build_pruned(name, precision, **kw):
    c = R.CASES[name]
    return build(c, precision, token_keep_rate=c["rate"], token_prune_blocks=c["blocks"], token_fuse=c["fuse"], **kw)


@pytest.mark.parametrize("precision", MODES)
def test_token_score_equals_the_attention_maps_bit_for_bit(precision):
    """mfvit_token_score on the qkv / lse a saved forward leaves behind (mfvit_vit_attn_layout) against get_attention_maps(mean, cls_only)."""
    c = R.CASES["two_stage96"]
    m = build(c, precision).eval()
    x = R.rng(961, (c["B"], 3) + c["hw"]).to(DEV)
    maps = m.get_attention_maps(x, blocks=[1], head_fusion="mean", cls_only=True)[0]
    cfg, ws, _ = m._rel_forward(x)
    lay = (ctypes.c_int64 * 4)()
    check(lib().mfvit_vit_attn_layout(cfg, lay), "mfvit_vit_attn_layout")
    B, T = c["B"], m.num_tokens
    bp, probs = guarded((B, T), torch.float32)
    bs, score = guarded((B, T - 1), torch.float32)
    check(lib().mfvit_token_score(int(lay[3]), ws.data_ptr() + lay[0] + lay[2], ws.data_ptr() + lay[1] + lay[2], B, T, c["heads"],
                                  c["dim"] // c["heads"], ptr(probs), ptr(score), stream()), "mfvit_token_score")
    torch.cuda.synchronize()
    assert band_untouched(bp, B * T) and band_untouched(bs, B * (T - 1))
    assert torch.equal(score, maps[:, 1:])
    m._release_ws(ws)


# --------------------------------------------------------------------------------------------------- block ranges through the C ABI
def seg_run(m, cfg, seg, x_in, dout, want_dimg=False, dparams=True, stages=None):
    """One forward + backward of a block range on fresh buffers: (x_out, gradient arena, dx_in / dimg)."""
    B, D = cfg.batch, m.embed_dim
    n = lib().mfvit_vit_workspace_bytes_seg(cfg, None, seg, int(want_dimg))
    assert n > 0
    ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    out = torch.empty(B, seg.tokens, D, device=DEV)
    check(lib().mfvit_vit_forward_seg(cfg, None, seg, ptr(m._arena), ptr(m._shadow), ptr(x_in), ptr(ws), ptr(out), stream()), "mfvit_vit_forward_seg")
    g = torch.zeros_like(m._arena) if dparams else None
    din = torch.empty(B, seg.tokens, D, device=DEV) if not seg.image_in else None
    dimg = torch.empty_like(x_in) if want_dimg else None
    for hi, lo in (stages or [(seg.block_hi, seg.block_lo - 1)]):
        check(lib().mfvit_vit_backward_seg(cfg, None, seg, ptr(m._arena), ptr(m._shadow), ptr(ws), ptr(dout), ptr(g), ptr(din),
                                           ptr(dimg) if lo == -1 else None, hi, lo, stream()), "mfvit_vit_backward_seg")
    torch.cuda.synchronize()
    return out, g, din if din is not None else dimg


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_full_range_equals_the_whole_stack_entry_points_bit_for_bit(precision):
    c = R.CASES["heads6_64"]
    m = build(c, precision).train()
    B, depth, T, D = c["B"], c["depth"], m.num_tokens, c["dim"]
    img = R.rng(971, (B, 3) + c["hw"]).to(DEV)
    dout = R.rng(972, (B, T, D)).to(DEV)
    cfg = m._cfg(img, True)
    m._ensure_shadow(cfg)
    # image input: mfvit_vit_forward + mfvit_vit_backward_ex
    ws = torch.empty(lib().mfvit_vit_workspace_bytes_ex(cfg, None, 1), device=DEV, dtype=torch.uint8)
    f0 = torch.empty(B, T, D, device=DEV)
    check(lib().mfvit_vit_forward(cfg, ptr(m._arena), ptr(m._shadow), ptr(img), ptr(ws), ptr(f0), stream()), "mfvit_vit_forward")
    g0, d0 = torch.zeros_like(m._arena), torch.empty_like(img)
    check(lib().mfvit_vit_backward_ex(cfg, None, ptr(m._arena), ptr(m._shadow), ptr(ws), ptr(dout), ptr(g0), ptr(d0), depth, -1, stream()),
          "mfvit_vit_backward_ex")
    seg = _lib.VitSeg(0, depth, T, 1)
    assert lib().mfvit_vit_workspace_bytes_seg(cfg, None, seg, 1) == ws.numel()
    f1, g1, d1 = seg_run(m, cfg, seg, img, dout, want_dimg=True)
    assert torch.equal(f0, f1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    # token input at a shortened sequence: mfvit_vit_forward_x0 + mfvit_vit_backward_x0
    Tk = 11
    x0, dk = R.rng(973, (B, Tk, D)).to(DEV), R.rng(974, (B, Tk, D)).to(DEV)
    ws = torch.empty(lib().mfvit_vit_workspace_bytes_x0(cfg, None, Tk), device=DEV, dtype=torch.uint8)
    f0 = torch.empty(B, Tk, D, device=DEV)
    check(lib().mfvit_vit_forward_x0(cfg, None, Tk, ptr(m._arena), ptr(m._shadow), ptr(x0), ptr(ws), ptr(f0), stream()), "mfvit_vit_forward_x0")
    g0, d0 = torch.zeros_like(m._arena), torch.empty_like(x0)
    check(lib().mfvit_vit_backward_x0(cfg, None, Tk, ptr(m._arena), ptr(m._shadow), ptr(ws), ptr(dk), ptr(g0), ptr(d0), depth, -1, stream()),
          "mfvit_vit_backward_x0")
    seg = _lib.VitSeg(0, depth, Tk, 0)
    assert lib().mfvit_vit_workspace_bytes_seg(cfg, None, seg, 0) == ws.numel()
    f1, g1, d1 = seg_run(m, cfg, seg, x0, dk)
    assert torch.equal(f0, f1) and torch.equal(g0, g1) and torch.equal(d0, d1)


@pytest.mark.parametrize("dim_case", ["heads6_64", "base768"])
@pytest.mark.parametrize("precision", MODES)
def test_a_stack_cut_into_two_ranges_matches_the_float64_reference(precision, dim_case):
    """Blocks [0, cut) on the image, then [cut, depth) on the first range's output, gradients chained back: features, every parameter gradient
    and d img inside CAPS (no bit equality: the second range enters through a LayerNorm row pass, not the fc2 epilogue)."""
    c = R.CASES[dim_case]
    m = build(c, precision).train()
    B, depth, T, D = c["B"], c["depth"], m.num_tokens, c["dim"]
    cut = 1
    p = R.case_params(c)
    img, r = R.rng(981, (B, 3) + c["hw"]), R.rng(982, (B, T, D))
    pd = {k: v.double().requires_grad_(k != "pos_embed") for k, v in p.items()}
    xi = img.double().requires_grad_(True)
    fr = ref_vit.features3d(pd, xi, c["heads"])
    (fr * r.double()).sum().backward()
    cfg = m._cfg(img, True)
    m._ensure_shadow(cfg)
    xd, rd = img.to(DEV), r.to(DEV)
    s0, s1 = _lib.VitSeg(0, cut, T, 1), _lib.VitSeg(cut, depth, T, 0)
    ws0 = torch.empty(lib().mfvit_vit_workspace_bytes_seg(cfg, None, s0, 1), device=DEV, dtype=torch.uint8)
    ws1 = torch.empty(lib().mfvit_vit_workspace_bytes_seg(cfg, None, s1, 0), device=DEV, dtype=torch.uint8)
    x1, f = torch.empty(B, T, D, device=DEV), torch.empty(B, T, D, device=DEV)
    a, sh = ptr(m._arena), ptr(m._shadow)
    check(lib().mfvit_vit_forward_seg(cfg, None, s0, a, sh, ptr(xd), ptr(ws0), ptr(x1), stream()), "mfvit_vit_forward_seg")
    check(lib().mfvit_vit_forward_seg(cfg, None, s1, a, sh, ptr(x1), ptr(ws1), ptr(f), stream()), "mfvit_vit_forward_seg")
    g, dx1, dimg = torch.zeros_like(m._arena), torch.empty_like(x1), torch.empty_like(xd)
    check(lib().mfvit_vit_backward_seg(cfg, None, s1, a, sh, ptr(ws1), ptr(rd), ptr(g), ptr(dx1), None, depth, cut - 1, stream()), "mfvit_vit_backward_seg")
    check(lib().mfvit_vit_backward_seg(cfg, None, s0, a, sh, ptr(ws0), ptr(dx1), ptr(g), None, ptr(dimg), cut, -1, stream()), "mfvit_vit_backward_seg")
    torch.cuda.synchronize()
    cap_f, cap_g = R.CAPS[precision]
    e_f, e_d = R.scale_err(f, fr), R.scale_err(dimg, xi.grad)
    worst = ("", 0.0)
    for k, (off, n) in m._offsets.items():
        if k == "pos_embed":
            continue
        e = R.scale_err(g[off:off + n].view(pd[k].shape), pd[k].grad)
        worst = (k, e) if e > worst[1] else worst
    print(f"two ranges [{dim_case},{precision}] features {e_f:.2e} worst grad {worst[0]} {worst[1]:.2e} dimg {e_d:.2e}")
    assert e_f < cap_f and worst[1] < cap_g and e_d < cap_g, (e_f, worst, e_d)


# --------------------------------------------------------------------------------------------------- the model
def model_step(m, name, token_indices=None, grads=True):
    """One forward + backward of the model on a case; patch dropout (explicit indices) is a training-mode front end: eval() runs the full grid."""
    _, img, pidx, r, rl = R.case_inputs(name, patch=m.training)
    x = img.to(DEV).requires_grad_(grads)
    kw = {}
    if pidx is not None and m.training:
        kw["keep_indices"] = pidx.to(DEV)
    if token_indices is not None:
        kw["token_indices"] = [t.to(DEV) for t in token_indices]
    for prm in m.parameters():
        prm.grad = None
    with torch.set_grad_enabled(grads):
        f = m.features3D(x, **kw)
        sel = [t.cpu() for t in m.last_token_indices]
        logits = m(x, **kw)
        if grads:
            ((f * r.to(DEV)).sum() + (logits * rl.to(DEV)).sum()).backward()
    return f, logits, sel, x


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_model_matches_the_restatement(name, precision, training):
    """Features, logits, every parameter gradient and d img against the float64 restatement run with the model's own selections; in fp32 and
    bf16x3 those selections are the float64 restatement's own, on every image and stage."""
    c = R.CASES[name]
    m = build_pruned(name, precision)
    m.train(training)
    f, logits, sel, x = model_step(m, name)
    sched = m.token_schedule(1 + c["patch_keep"] if (c["patch_keep"] and training) else None)
    assert f.shape == (c["B"], sched[-1], c["dim"]) and len(sel) == len(sched) - 1
    own = R.reference(name, patch=training)
    if precision in ("fp32", "bf16x3"):
        assert len(own["indices"]) == len(sel) and all(torch.equal(a, b) for a, b in zip(own["indices"], sel)), "selection differs from float64"
    ref = own if all(torch.equal(a, b) for a, b in zip(own["indices"], sel)) else R.run(name, torch.float64, indices=sel, patch=training)
    cap_f, cap_g = R.CAPS[precision]
    e_f, e_l, e_d = R.scale_err(f, ref["features"]), R.scale_err(logits, ref["logits"]), R.scale_err(x.grad, ref["dimg"])
    worst = ("", 0.0)
    for k, prm in m.named_parameters():
        if k == "pos_embed":
            assert prm.grad is None
            continue
        e = R.scale_err(prm.grad, ref["grads"][k])
        worst = (k, e) if e > worst[1] else worst
    print(f"{name}[{precision},train={int(training)}] features {e_f:.2e} logits {e_l:.2e} worst grad {worst[0]} {worst[1]:.2e} dimg {e_d:.2e}")
    m.check_keep_error()
    assert e_f < cap_f and e_l < cap_f and worst[1] < cap_g and e_d < cap_g, (e_f, e_l, worst, e_d)
    org = R.token_origin(sel, sched[0], c["fuse"])
    assert torch.equal(m.token_origin().cpu(), org)


def test_forced_token_indices_are_honoured():
    name = "two_stage96"
    c = R.CASES[name]
    m = build_pruned(name, "bf16x3").train()
    sched = m.token_schedule()
    g = torch.Generator().manual_seed(5)
    forced = [torch.stack([torch.randperm(T - 1, generator=g)[:Tn - 2] for _ in range(c["B"])]) for T, Tn in zip(sched, sched[1:])]
    f, logits, sel, x = model_step(m, name, token_indices=forced)
    assert all(torch.equal(a, b.sort(dim=1)[0]) for a, b in zip(sel, forced))
    ref = R.run(name, torch.float64, indices=forced)
    cap_f, cap_g = R.CAPS["bf16x3"]
    assert R.scale_err(f, ref["features"]) < cap_f and R.scale_err(x.grad, ref["dimg"]) < cap_g
    e = max(R.scale_err(prm.grad, ref["grads"][k]) for k, prm in m.named_parameters() if prm.grad is not None)
    assert e < cap_g, e
    # the model's own selection, handed back, reproduces the run bit for bit
    # (one encoder pass per run: model_step's second call shares the first's node only without forced indices)
    _, img, _, r, _ = R.case_inputs(name)

    def one_pass(token_indices):
        xx = img.to(DEV).requires_grad_(True)
        ff = m.features3D(xx, token_indices=token_indices)
        (ff * r.to(DEV)).sum().backward()
        return ff.detach(), xx.grad, [t.clone() for t in m.last_token_indices]
    f1, d1, sel1 = one_pass(None)
    f2, d2, sel2 = one_pass(sel1)
    assert torch.equal(f1, f2) and torch.equal(d1, d2) and all(torch.equal(a, b) for a, b in zip(sel1, sel2))
    for bad in ([forced[0]], [forced[0][:, :-1], forced[1]], [forced[0].float(), forced[1]], [forced[0] + 30, forced[1]],
                [forced[0][:, [0] * forced[0].shape[1]], forced[1]]):
        with pytest.raises(MfvitError):
            m.features3D(x.detach(), token_indices=bad)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_rate_one_gives_the_bits_of_a_model_without_the_arguments(precision):
    c = R.CASES["heads6_64"]
    m0 = build(c, precision).train()
    m1 = build(c, precision, token_keep_rate=1.0, token_prune_blocks=c["blocks"], token_fuse=True).train()
    calls = []
    real = m1._forward_chain                        # (img, idx, plan, ..): a pruned forward is one with more than one block range
    m1._forward_chain = lambda *a, **k: (len(a[2]) > 1 and calls.append(1)) or real(*a, **k)
    img, r = R.rng(991, (c["B"], 3) + c["hw"]), R.rng(992, (c["B"], m0.num_tokens, c["dim"]))
    outs = []
    for m in (m0, m1):
        x = img.to(DEV).requires_grad_(True)
        f = m.features3D(x)
        (f * r.to(DEV)).sum().backward()
        outs.append([f.detach(), x.grad] + [prm.grad for prm in m.parameters() if prm.grad is not None])
    assert calls == [] and len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs))
    m1.token_keep_rate = 0.7                        # a plain attribute: the next forward prunes
    assert m1.features3D(img.to(DEV)).shape[1] == m1.token_schedule()[-1] < m0.num_tokens and calls == [1]


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_a_sample_does_not_depend_on_its_batch_and_two_runs_agree(precision):
    """Image b alone gives the bits it gives inside the batch (features; d img in bf16x3 - in fp32 the unchanged data-gradient chain of the block
    stack is itself not bit-stable against the batch, tests/test_patch_drop_gpu.py, so d img is held to the 1e-5 of that test), and two identical
    calls give identical bits."""
    name = "two_stage96"
    c = R.CASES[name]
    m = build_pruned(name, precision).train()
    _, img, _, r, _ = R.case_inputs(name)

    def go(sel):
        x = img[sel].contiguous().to(DEV).requires_grad_(True)
        for prm in m.parameters():
            prm.grad = None
        f = m.features3D(x)
        (f * r[sel].to(DEV)).sum().backward()
        return f.detach(), x.grad.detach(), [prm.grad.clone() for prm in m.parameters() if prm.grad is not None]
    f_all, d_all, g_all = go(slice(0, c["B"]))
    f_2, d_2, g_2 = go(slice(0, c["B"]))
    assert torch.equal(f_all, f_2) and torch.equal(d_all, d_2) and all(torch.equal(a, b) for a, b in zip(g_all, g_2))
    for b in range(c["B"]):
        f_b, d_b, _ = go(slice(b, b + 1))
        assert torch.equal(f_all[b:b + 1], f_b), b
        if precision == "fp32":
            assert R.scale_err(d_all[b:b + 1], d_b) < 1e-5, b
        else:
            assert torch.equal(d_all[b:b + 1], d_b), b


def pooled_bytes(m):
    return sum(t.numel() for pool in m._ws_pool.values() for t in pool)


def test_a_rate_warm_up_keeps_the_workspace_pool_bounded():
    """token_keep_rate stepped through ten values (EViT warms it up), a train step and an eval() forward at each: every rate has range workspaces
    of its own sizes, and the pool must hold those of the CURRENT plan only - at most two buffers per size in use (the pool's own cap), whatever
    came before.  Also here: token_origin() composes with the fuse flag of the forward it describes, not with the attribute's later value."""
    name = "two_stage96"
    c = R.CASES[name]
    m = build_pruned(name, "bf16x3").train()
    _, img, _, _, _ = R.case_inputs(name)
    x = img.to(DEV)
    seen = set()
    for rate in (0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6, 0.55, 0.5, 0.45):
        m.token_keep_rate = rate
        m.train()
        m.features3D(x).sum().backward()
        m.zero_grad(set_to_none=True)
        m.eval()
        with torch.no_grad():
            m.features3D(x)
        live = set().union(*m._prune_sizes.values())
        seen |= live
        held = {n for n, pool in m._ws_pool.items() if pool}
        assert held <= live, (rate, sorted(held - live))
        assert pooled_bytes(m) <= 2 * sum(live), (rate, pooled_bytes(m), sum(live))
    # (the check can tell: a pool that kept every size ever used would hold at least sum(seen) bytes by now)
    assert len(seen) >= 20 and sum(seen) > 2 * sum(live) >= pooled_bytes(m), (len(seen), sum(seen), sum(live), pooled_bytes(m))
    sel = [t.cpu() for t in m.last_token_indices]
    org = R.token_origin(sel, m.num_tokens, True)
    m.token_fuse = False
    assert torch.equal(m.token_origin().cpu(), org)


def test_frozen_backbone_returns_the_image_gradient_only():
    name = "two_stage96"
    m = build_pruned(name, "bf16x3").train()
    for prm in m.parameters():
        prm.requires_grad_(False)
    f, logits, sel, x = model_step(m, name)
    ref = R.reference(name)
    assert all(prm.grad is None for prm in m.parameters())
    assert R.scale_err(x.grad, ref["dimg"]) < R.CAPS["bf16x3"][1]


@pytest.mark.parametrize("bucket", [1, 2, 4])
def test_stage_hook_sees_descending_model_stages_once_each(bucket):
    name = "two_stage96"
    c = R.CASES[name]
    m = build_pruned(name, "fp32").train()
    _, _, _, x0 = model_step(m, name)
    ref = {k: prm.grad.clone() for k, prm in m.named_parameters() if prm.grad is not None}
    ref["d img"] = x0.grad.clone()
    seen = []
    m._grad_bucket_layers = bucket
    m._grad_stage_hook = lambda vit, hi, lo, gflat: seen.append((hi, lo))
    _, _, _, x1 = model_step(m, name)
    del m._grad_stage_hook
    assert [s for hi, lo in seen for s in range(hi, lo - 1, -1)] == list(range(c["depth"], -2, -1)), seen
    got = {k: prm.grad for k, prm in m.named_parameters() if prm.grad is not None}
    got["d img"] = x1.grad
    assert set(got) == set(ref)
    for k in ref:
        assert R.scale_err(got[k], ref[k]) < 1e-5, k


def test_dropout_and_drop_path_with_pruning_features():
    """Training-mode dropout sites and drop path on a pruned sequence: features against the restatement fed the kernels' own masks
    (mfvit_dropout_mask at each range's sequence length: sites keep the model's block numbers, sample = row / tokens)."""
    from mfvit import ops
    c = dict(R.CASES["two_stage96"])
    rates = dict(drop_rate=0.1, attn_drop_rate=0.15, drop_path_rate=0.4)
    m = build(c, "bf16x3", token_keep_rate=c["rate"], token_prune_blocks=c["blocks"], token_fuse=True, **rates).train()
    _, img, _, _, _ = R.case_inputs("two_stage96")
    torch.manual_seed(3)
    f = m.features3D(img.to(DEV))
    sel = [t.cpu() for t in m.last_token_indices]
    drop, attn, dpr = m.drop_rates()
    seed = m._last_drop.seed
    B, D, F, H = c["B"], c["dim"], 4 * c["dim"], c["heads"]
    mk = {}

    def get(p, site, n, shape):
        return ops.dropout_mask(p, seed, site, n).reshape(shape).double().cpu()
    segs = m._token_segments(m.num_tokens)
    mk["pos"] = get(drop, 1, B * segs[0][2] * D, (B, segs[0][2], D))
    for lo, hi, T in segs:
        for l in range(lo, hi):
            mk["attn", l] = get(attn, 16 * l + 2, B * H * T * T, (B, H, T, T))
            mk["proj", l] = get(drop, 16 * l + 3, B * T * D, (B, T, D))
            mk["fc2", l] = get(drop, 16 * l + 4, B * T * D, (B, T, D))
            mk["gelu", l] = get(drop, 16 * l + 5, B * T * F, (B, T, F))
            if dpr[l] > 0:
                mk["dp_attn", l] = get(dpr[l], 16 * l + 6, B, (B, 1, 1))
                mk["dp_mlp", l] = get(dpr[l], 16 * l + 7, B, (B, 1, 1))
    pd = {k: v.double() for k, v in R.case_params(c).items()}
    with torch.no_grad():
        fr, _ = R.features3d_pruned(pd, img.double(), c["blocks"], c["rate"], True, indices=sel, heads=H, masks=mk, rates=(drop, attn, dpr))
    e = R.scale_err(f, fr)
    print(f"dropout + drop path + pruning [bf16x3] features {e:.2e}")
    assert e < R.CAPS["bf16x3"][0], e


# --------------------------------------------------------------------------------------------------- Fus_CrossViT and the refusals
def build_fus(rate_c, rate_e, blocks_e=(0,), depth=2, hw=(64, 64), precision="bf16x3"):
    fus = importlib.import_module(FUS_MOD)
    import vits
    backs = []
    for i, (rate, blocks) in enumerate(((rate_c, (0,)), (rate_e, blocks_e))):
        m = vits.vit_small(num_classes=3, depth=depth, precision=precision, img_size=hw, token_keep_rate=rate, token_prune_blocks=blocks)
        m.load_state_dict(R.P.params_for(9961 + i, hw, depth))
        backs.append(m.to(DEV).train())
    model = fus.Fus_CrossViT(backs[0], backs[1])
    fp = ref_fusion.seeded_fusion_params(9963)
    model.load_state_dict(fp)
    return model.to(DEV).train(), backs, fp


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_fus_crossvit_on_pruned_encoders(precision):
    """End to end against the float64 fusion oracle fed the float64 pruned features (the models' own selections), inside
    fusion_edges_ref.GATES - with fp32 encoders: those gates are the f32 exchange's own error on identical features (4 x 5.6e-7), and an
    encoder whose own forward error is above them (bf16x3: 1e-5 measured on these features, 2e-5 documented) cannot meet them whatever the
    pruning does.  In bf16x3, the default, the exchange is therefore fed the encoders' own pruned features (the form of
    tests/test_patch_drop_gpu.py) and the features themselves are held to CAPS."""
    B = 3
    model, (vc, ve), fp = build_fus(0.5, 0.5, precision=precision)
    x, xe = R.rng(9971, (B, 3, 64, 64)).to(DEV), R.rng(9972, (B, 3, 64, 64)).to(DEV)
    fused, x_c, x_e = model(vc, ve, x, xe)
    ic, ie = vc.last_token_indices, ve.last_token_indices
    assert ic[0].shape == ie[0].shape == (B, 8) and not torch.equal(ic[0], ie[0])        # each stream selects by its own attention
    (fused + x_c + x_e).sum().backward()
    for vit in (vc, ve):
        assert all(prm.grad is not None and torch.isfinite(prm.grad).all() and float(prm.grad.abs().max()) > 0
                   for k, prm in vit.named_parameters() if k != "pos_embed" and not k.startswith("head")), "encoder gradients"
    # the float64 pruned features of both streams (the models' own selections) through the float64 fusion oracle
    feats = []
    for vit, img, seed in ((vc, x, 9961), (ve, xe, 9962)):
        pd = {k: v.double() for k, v in R.P.params_for(seed, (64, 64), 2).items()}
        with torch.no_grad():
            f, _ = R.features3d_pruned(pd, img.double().cpu(), (0,), 0.5, True, indices=[t.cpu() for t in vit.last_token_indices])
        feats.append(f)
    if precision != "fp32":
        with torch.no_grad():
            own = [vit.features3D(img, token_indices=vit.last_token_indices) for vit, img in ((vc, x), (ve, xe))]
        e_feat = [R.scale_err(a, b) for a, b in zip(own, feats)]
        print(f"Fus_CrossViT [{precision}] pruned features against float64: {e_feat}")
        assert max(e_feat) < R.CAPS[precision][0], e_feat
        feats = [t.double().cpu() for t in own]
    pdf = {k: v.double() for k, v in fp.items()}
    r_fused, r_c, r_e = ref_fusion.fus_ex_forward(pdf, feats[0], feats[1], hw_cxr=vc.head.weight.detach().double().cpu(),
                                                  hb_cxr=vc.head.bias.detach().double().cpu(), hw_enh=ve.head.weight.detach().double().cpu(),
                                                  hb_enh=ve.head.bias.detach().double().cpu())
    errs = [R.scale_err(a, b) for a, b in ((fused, r_fused), (x_c, r_c), (x_e, r_e))]
    print(f"Fus_CrossViT on pruned tokens [{precision}]: fused / x_cxr / x_enh {errs}")
    assert max(errs) < FUSION_GATES["out"], errs
    # gradients of the exchange through the same comparison: the loss of the step above, on the oracle fed the same features
    pg = {k: v.double().requires_grad_(True) for k, v in fp.items()}
    o = ref_fusion.fus_ex_forward(pg, feats[0], feats[1], hw_cxr=vc.head.weight.detach().double().cpu(), hb_cxr=vc.head.bias.detach().double().cpu(),
                                  hw_enh=ve.head.weight.detach().double().cpu(), hb_enh=ve.head.bias.detach().double().cpu())
    (o[0] + o[1] + o[2]).sum().backward()
    named = dict(model.named_parameters())
    for k, q in (("multi_scale_transformers.0.cross_attn_layers.0.0.fn.wk.weight", "d.wk"),
                 ("multi_scale_transformers.0.cross_attn_layers.0.0.fn.wv.weight", "d.wv")):
        e = R.scale_err(named[k].grad, pg[k].grad)
        print(f"Fus_CrossViT on pruned tokens [{precision}]: {q} {e:.2e} (gate {FUSION_GATES[q]:.0e})")
        assert e < FUSION_GATES[q], (k, e)


def test_fus_crossvit_refuses_a_mismatched_pair():
    x = R.rng(9981, (2, 3, 64, 64)).to(DEV)
    for rc, re_, be, word in ((0.5, 0.7, (0,), "token_keep_rate"), (0.5, 1.0, (0,), "one encoder"), (0.5, 0.5, (0, 1), "token_prune_blocks")):
        model, (vc, ve), _ = build_fus(rc, re_, be, depth=3)
        with pytest.raises(MfvitError, match=word):
            model(vc, ve, x, x)


def test_refusals_while_pruning_is_active():
    from mfvit import lora, similarity
    c = R.CASES["heads6_64"]
    m = build_pruned("heads6_64", "bf16x3").eval()
    x = R.rng(9991, (2, 3) + c["hw"]).to(DEV)
    for call in (lambda: m.get_attention_maps(x), lambda: m.attention_rollout(x), lambda: m.attention_relevance(x),
                 lambda: m.get_relevance_maps(x), lambda: m.attention_stats(x), lambda: m.hidden_states(x),
                 lambda: m.get_intermediate_layers(x), lambda: similarity.cka(m, m, [x], unbiased=False)):
        with pytest.raises(MfvitError, match="token"):
            call()
    model, (vc, ve), _ = build_fus(0.5, 0.5)
    for call in (lambda: model.attention_relevance(vc, ve, x, x), lambda: model.get_exchange_attention(vc, ve, x, x),
                 lambda: model.cross_relevance(vc, ve, x, x)):
        with pytest.raises(MfvitError, match="token"):
            call()
    lora.add_lora(m, rank=4)
    with pytest.raises(MfvitError, match="LoRA"):
        m.features3D(x)
    lora.remove_lora(m)
    m.token_keep_rate = 1.0                         # lifted with the rate
    assert len(m.get_attention_maps(x)) == c["depth"]
