"""GPU parity of the ViT-S/16 encoder (vits.vit_small -> mfvit_vit_forward / mfvit_vit_backward) against the CPU
oracle (oracle/ref_vit.py) on identical seeded weights and inputs.

Tolerances:
  precision='fp32' : BASELINE.json north_star - outputs within 1e-3 relative of the f32 CPU path, argmax bit-exact.
                     (exact-f32 MFMA; measured error is ~1e-5, asserted at 1e-3 / 2e-3 for gradients)
  precision='bf16' : bf16 operands with f32 accumulation through 12 blocks: asserted at 4e-2 of the output scale
                     (features are LayerNorm outputs of O(1)); the measured value is logged to gpurun_out/.
"""
import os

import pytest
import torch

from conftest import rng_tensor
from oracle import ref_vit

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_encoder.txt")


def log(msg):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")


def build(precision, seed, depth=12, num_classes=3, img=224, **kw):
    import vits
    m = vits.vit_small(num_classes=num_classes, depth=depth, precision=precision, img_size=img, **kw)
    p = ref_vit.seeded_params(seed, num_classes=num_classes, depth=depth, img_size=img)
    missing = m.load_state_dict(p, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to("cuda:0"), p


def scale_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 4e-2)])
@pytest.mark.parametrize("B,img", [(2, 224), (1, 384), (3, 64)])
def test_features3d_and_logits(precision, tol, B, img):
    m, p = build(precision, 501, img=img)
    x = rng_tensor(502, (B, 3, img, img))
    with torch.no_grad():
        ref_f = ref_vit.features3d(p, x)
        ref_l = ref_vit.head_linear(p, ref_f[:, 0])
        xg = x.to("cuda:0")
        f = m.features3D(xg)
        logits = m(xg)
    assert f.shape == ref_f.shape and f.dtype == torch.float32
    e_f, e_l = scale_err(f, ref_f), scale_err(logits, ref_l)
    log(f"features3D[{precision},B={B},img={img}] err={e_f:.3e} logits err={e_l:.3e}")
    assert e_f < tol and e_l < tol
    if precision == "fp32":
        assert logits.argmax(1).cpu().tolist() == ref_l.argmax(1).tolist()


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-3), ("bf16", 6e-2)])
@pytest.mark.parametrize("stop_grad_conv1", [False, True])
def test_backward_all_parameters(precision, tol, stop_grad_conv1):
    B, depth = 2, 3
    m, p = build(precision, 511, depth=depth, stop_grad_conv1=stop_grad_conv1)
    x = rng_tensor(512, (B, 3, 224, 224))
    r = rng_tensor(513, (B, 197, 384))
    rl = rng_tensor(514, (B, 3))
    pd = {k: v.double().requires_grad_(k != "pos_embed") for k, v in p.items()}
    f_ref = ref_vit.features3d(pd, x.double())
    loss_ref = (f_ref * r.double()).sum() + (ref_vit.head_linear(pd, f_ref[:, 0]) * rl.double()).sum()
    loss_ref.backward()
    xg = x.to("cuda:0")
    f = m.features3D(xg)
    loss = (f * r.to("cuda:0")).sum() + (m(xg) * rl.to("cuda:0")).sum()
    loss.backward()
    worst = ("", 0.0)
    for name, prm in m.named_parameters():
        if name == "pos_embed":
            assert prm.grad is None
            continue
        if stop_grad_conv1 and name.startswith("patch_embed"):
            assert prm.grad is None
            continue
        assert prm.grad is not None, name
        e = scale_err(prm.grad, pd[name].grad)
        if e > worst[1]:
            worst = (name, e)
        assert e < tol, (name, e)
    log(f"backward[{precision},stop_grad_conv1={stop_grad_conv1}] worst {worst[0]} err={worst[1]:.3e}")


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16", "fp32"])
def test_full_size_batch_is_sample_independent(precision):
    """BASELINE configs[2] size (B = 128 at 224^2, M = 25,216 token rows - too big for the CPU oracle): a ViT has no cross-sample
    op, so every sample of the full batch must come out exactly as it does in the small batches the oracle tests cover (the GEMM
    tiles, attention workgroups and row kernels may not leak between rows, pad rows or tile tails).  Forward: bit-exact in fp32; in the
    16-bit modes the row-complete GEMMs switch kernels with the row count (two workgroups per CU above 16,384 token rows; in the default
    split-bf16 precision the tall-tile kernel of gemm_rowp.hip above 4,096: other MFMA shape, other summation order), so an f32 last-bit
    difference can flip a rounding of the operand type: the rows must agree to a few ulps of THAT type - 1e-4 for split bf16 (16
    mantissa bits: a flipped hi rounding is absorbed by the lo part), 1e-2 for bf16, 2e-3 for fp16; a leak between rows, pad rows or tile
    tails would be an O(1) error.  Backward:
    the input-independent reduction order of the split-M weight gradients changes with M, so the full-batch gradient is compared
    with the SUM of the sub-batch gradients at rounding level."""
    m, _ = build(precision, 601, depth=2 if precision == "fp32" else 12)
    B = 128
    x = rng_tensor(602, (B, 3, 224, 224)).to("cuda:0")
    with torch.no_grad():
        full = m.features3D(x)
        for lo, n in ((0, 4), (60, 3), (125, 3)):                   # first, middle and the tail rows of the last M-tile
            part = m.features3D(x[lo:lo + n].contiguous())
            if precision == "fp32":
                assert torch.equal(full[lo:lo + n], part), (precision, lo)
            else:
                e = ((full[lo:lo + n] - part).abs().max() / part.abs().max()).item()
                assert e < {"bf16x3": 1e-4, "bf16": 1e-2, "fp16": 2e-3}[precision], (precision, lo, e)
    assert torch.isfinite(full).all()
    # gradient linearity over the batch: grad(sum over 128) == grad(first 64) + grad(last 64)
    w = rng_tensor(603, (B, 197, 384)).to("cuda:0")

    def grads(lo, hi):
        for p_ in m.parameters():
            p_.grad = None
        (m.features3D(x[lo:hi].contiguous()) * w[lo:hi]).sum().backward()
        return {k: p_.grad.detach().clone() for k, p_ in m.named_parameters() if p_.grad is not None}

    g_all, g_a, g_b = grads(0, B), grads(0, 64), grads(64, B)
    # 16-bit modes: dY is rounded to the operand type per call, so the sums differ by its rounding (split bf16: 2^-17, but gelu' rides in
    # plain fp16 - see DESIGN.md 2)
    tol = {"bf16": 2e-2, "fp16": 5e-3, "bf16x3": 1e-3, "fp32": 1e-4}[precision]
    worst = 0.0
    for k in g_all:
        e = scale_err(g_all[k], g_a[k] + g_b[k])
        worst = max(worst, e)
        assert e < tol, (k, e)
    log(f"full-size batch independence [{precision}]: forward {'bit-exact' if precision == 'fp32' else 'to a few ulps'}, gradient additivity worst {worst:.2e}")


@pytest.mark.parametrize("bucket", [1, 4, 5])
def test_grouped_backward_stages_match_single_call(bucket):
    """The data-parallel path runs the encoder backward in groups of stages (one library call + one gradient bucket per group,
    mfvit/ddp.py); every grouping must give the gradients of the single-call backward and cover every stage exactly once."""
    m, _ = build("fp32", 611, depth=12)
    x = rng_tensor(612, (2, 3, 224, 224)).to("cuda:0")
    w = rng_tensor(613, (2, 197, 384)).to("cuda:0")

    def grads():
        for p_ in m.parameters():
            p_.grad = None
        (m.features3D(x) * w).sum().backward()
        return {k: p_.grad.detach().clone() for k, p_ in m.named_parameters() if p_.grad is not None}

    ref = grads()
    seen = []
    m._grad_bucket_layers = bucket
    m._grad_stage_hook = lambda vit, hi, lo, gflat: seen.append((hi, lo))
    got = grads()
    del m._grad_stage_hook
    stages = [s for hi, lo in seen for s in range(hi, lo - 1, -1)]
    assert stages == list(range(12, -2, -1)), seen                  # final norm, blocks 11..0, embedding: each once, in order
    for k in ref:
        assert scale_err(got[k], ref[k]) < 1e-5, k


def test_gradient_arena_reuse_is_safe():
    """The flat gradient arena is reused from step to step (stable addresses for the optimizers' device tables).  It must NOT be
    reused while a gradient still lives in it: accumulation over two backward passes without zero_grad, and two passes through the
    same encoder inside ONE autograd run (what MoCo-v3 does) - both must equal the sum of the separate gradients."""
    m, _ = build("fp32", 621, depth=2)
    xa = rng_tensor(622, (2, 3, 224, 224)).to("cuda:0")
    xb = rng_tensor(623, (2, 3, 224, 224)).to("cuda:0")
    w = rng_tensor(624, (2, 197, 384)).to("cuda:0")

    def zero():
        for p_ in m.parameters():
            p_.grad = None

    def snap():
        return {k: p_.grad.detach().clone() for k, p_ in m.named_parameters() if p_.grad is not None}

    zero(); (m.features3D(xa) * w).sum().backward(); ga = snap()
    ptr_a = m.blocks[0].mlp.fc1.weight.grad.data_ptr()
    zero(); (m.features3D(xb) * w).sum().backward(); gb = snap()
    assert m.blocks[0].mlp.fc1.weight.grad.data_ptr() == ptr_a            # reused: same addresses step after step
    zero()
    (m.features3D(xa) * w).sum().backward()
    (m.features3D(xb) * w).sum().backward()                                # accumulates into the live gradients
    acc = snap()
    zero()
    ((m.features3D(xa) * w).sum() + (m.features3D(xb) * w).sum()).backward()   # two passes in one autograd run
    both = snap()
    for k in ga:
        want = ga[k] + gb[k]
        assert scale_err(acc[k], want) < 1e-5, k
        assert scale_err(both[k], want) < 1e-5, k


def test_state_dict_roundtrip_and_arena_survives_moves():
    m, p = build("fp32", 521, depth=2)
    sd = m.state_dict()
    assert set(sd.keys()) == set(p.keys())
    for k in p:
        assert torch.equal(sd[k].cpu(), p[k]), k
    assert m._arena_intact() and m.flat_parameters().is_cuda
    with torch.no_grad():
        m.blocks[1].mlp.fc1.weight.mul_(0.5)            # in-place update is seen through the arena
    off, n = m.arena_slice("blocks.1.mlp.fc1.weight")
    assert torch.equal(m.flat_parameters()[off:off + n].view(1536, 384).cpu(), p["blocks.1.mlp.fc1.weight"] * 0.5)


def test_cpu_input_fails_loudly():
    from mfvit import MfvitError
    m, _ = build("fp32", 531, depth=1)
    with pytest.raises(MfvitError):
        m(torch.zeros(1, 3, 224, 224))


def test_default_1000_class_head_runs_on_the_hip_head_kernels():
    """vits.vit_small() keeps timm's default 1000-way head; its forward / backward go through mfvit_head_fwd / _bwd (row-dot kernels
    over the cls rows), not through a library GEMM - checked against the oracle's head on the same weights."""
    m, p = build("bf16x3", 541, depth=1, num_classes=1000)
    x = rng_tensor(542, (3, 3, 224, 224))
    logits = m(x.to("cuda:0"))
    assert logits.shape == (3, 1000) and type(logits.grad_fn).__name__ == "_HeadFnBackward"
    pd = {k: v.double().requires_grad_(k.startswith("head")) for k, v in p.items()}
    ref = ref_vit.head_linear(pd, ref_vit.features3d(pd, x.double())[:, 0])
    assert scale_err(logits, ref) < 1e-3
    r = rng_tensor(543, (3, 1000))
    (logits * r.to("cuda:0")).sum().backward()
    (ref * r.double()).sum().backward()
    assert scale_err(m.head.weight.grad, pd["head.weight"].grad) < 1e-3 and scale_err(m.head.bias.grad, pd["head.bias"].grad) < 1e-3


@pytest.mark.parametrize("B", [16, 3, 96])
def test_gradients_are_bit_identical_from_run_to_run(B):
    """Every sum of the encoder backward is taken in a FIXED order: three backward passes over the same forward give the SAME BITS for EVERY parameter gradient.
    Round 5 (VERDICT r4 task 5): the weight-gradient GEMMs leave their split partials as plain stores and a batched reduce adds them in a fixed order - the 2-D
    gradients, 99.9 % of the parameters.  Round 6: the 1-D ones too - LayerNorm weights / biases and the proj / fc2 biases (column partials of the row kernels:
    one block adds all partial rows of its columns, gemm.hip::colpart_reduce), the qkv bias (ones-fragment sums of the weight-gradient kernels: one row of
    partials per split, reduced with the tiles), the fc1 bias (column sums of the x gelu' tile epilogue: one row of partials per 64-row block), cls_token and the
    patch-embedding bias (colsum_rows: one block per 64 columns) - and the forward itself (the persistent attention kernel moved ~2 % of its rows by a rounding
    from run to run until round 6, see tests/test_precision_gpu.py).  B = 16: M = 3,152 (LDS-DMA weight gradients, paired dWqkv + dWproj launch, K-split row
    kernels); B = 3: M = 591 (gemm_tn); B = 96: M = 18,912 (the persistent attention kernels, the ping-pong tile GEMM)."""
    import vits
    depth = 2
    m = vits.vit_small(num_classes=0, depth=depth, precision="bf16x3")
    m.load_state_dict(ref_vit.seeded_params(611, num_classes=0, depth=depth), strict=False)
    m = m.to("cuda:0")
    x = rng_tensor(612, (B, 3, 224, 224)).to("cuda:0")
    w = rng_tensor(613, (B, 197, 384)).to("cuda:0")
    runs = []
    for _ in range(3):
        m.zero_grad(set_to_none=True)
        f = m.features3D(x)
        (f * w).sum().backward()
        torch.cuda.synchronize()
        g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        g["features"] = f.detach().clone()
        runs.append(g)
    assert len(runs[0]) == 12 * depth + 5 + 1, sorted(runs[0])        # 12 per block; cls_token, patch embedding w / b, final norm w / b (pos_embed: a fixed table); features
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]) and torch.equal(runs[0][n], runs[2][n]), n


def test_attention_backward_scale_from_the_proj_gradient_epilogue(monkeypatch):
    """Round 6: the split-fp16 attention backward takes the power-of-two scale of every (image, head) pair from maxima the proj data-gradient GEMM leaves
    behind (GemmP::omax, csrc/gemm.hip -> attn_bwd_sp_kernel<.., DM = true>) instead of prefetching dO's hi parts itself (MFVIT_DO_MAX=0).  Both paths must
    pick the SAME exponent for every pair (the producer's f32 maximum is rounded to bf16 like the hi parts the prefetch sees), so every 2-D weight gradient -
    deterministic sums, see the test above - is the same bits either way; the 1-D ones (float atomics) agree to rounding.  B = 96: 1,152 pairs (the
    single-pass kernel runs), M = 18,912 rows = 147.75 GEMM tiles (the last one partial), 64-row wave slices that straddle image boundaries.  The upstream
    gradient's magnitude varies by six orders from image to image: a maximum filed under a neighbouring image or head would be off by up to 2^20."""
    import vits
    depth, B = 2, 96
    m = vits.vit_small(num_classes=0, depth=depth, precision="bf16x3")
    m.load_state_dict(ref_vit.seeded_params(621, num_classes=0, depth=depth), strict=False)
    m = m.to("cuda:0")
    x = rng_tensor(622, (B, 3, 224, 224)).to("cuda:0")
    mag = 10.0 ** (torch.arange(B, dtype=torch.float32) * 7 % 6 - 4.0)                 # 1e-4 .. 1e+1, neighbours far apart
    w = (rng_tensor(623, (B, 197, 384)) * mag.view(B, 1, 1)).to("cuda:0")
    grads = {}
    for sw in ("1", "0", "1"):
        monkeypatch.setenv("MFVIT_DO_MAX", sw)                                         # (conftest.py: MFVIT_AB_LIVE=1, read at every call)
        m.zero_grad(set_to_none=True)
        (m.features3D(x) * w).sum().backward()
        torch.cuda.synchronize()
        grads.setdefault(sw, []).append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    a, b, a2 = grads["1"][0], grads["0"][0], grads["1"][1]
    two_d = [n for n, g in a.items() if g.ndim >= 2 and n != "cls_token"]
    assert len(two_d) == 4 * depth + 1
    worst = 0.0
    for n in a:
        assert torch.isfinite(a[n]).all(), n
        if n in two_d:
            assert torch.equal(a[n], a2[n]), n                 # (the maxima buffer is zeroed by every call: nothing left over from the call before)
            assert torch.equal(a[n], b[n]), (n, scale_err(a[n], b[n]))
        worst = max(worst, scale_err(a[n], b[n]), scale_err(a2[n], b[n]))
    log(f"attention backward scale from the proj-gradient epilogue vs the prefetch path: {len(two_d)} weight gradients bit-identical, worst 1-D gradient "
        f"difference {worst:.2e} (B = {B}, depth {depth})")
    assert worst < 1e-4, worst


# --------------------------------------------------------------------------------------------------- the one forward / backward chain
# features3D runs every forward as block ranges through mfvit_vit_forward_seg / _backward_seg (mfvit/encoder.py, _forward_chain / _backward_chain).
# The range [0, depth) issues the launches of the whole-stack and given-x0 entry points in the same order (include/mfvit.h; pinned on the CPU by
# tests/test_encoder_trace_cpu.py), and every sum has a fixed order: the results are the same bits.  B = 2, 64 x 64 (T = 17), depth 2, 6 heads.
CHAIN_PRECISIONS = ["bf16x3", "fp32"]


def _chain_case(precision, seed, **kw):
    m, _ = build(precision, seed, depth=2, img=64, **kw)
    x = rng_tensor(seed + 1, (2, 3, 64, 64)).to("cuda:0")
    return m.train(), x


def _through_model(m, x, r, **kw):
    """(features, gradient arena, d img) of features3D with every parameter trainable and the image requiring a gradient"""
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    f = m.features3D(xg, **kw)
    (f * r).sum().backward()                            # (d / d features = r, the same bits)
    torch.cuda.synchronize()
    return f.detach().clone(), m._last_grad_arena.clone(), xg.grad.clone()


def _whole_stack_calls(m, x, r, drop):
    """The same through mfvit_vit_forward(_drop) + mfvit_vit_backward_ex on fresh buffers, the model's arena and shadow."""
    from mfvit._lib import check, lib, ptr, stream
    cfg = m._cfg(x, True)
    m._ensure_shadow(cfg)
    h, arena = lib(), m.flat_parameters()
    ws = torch.empty(h.mfvit_vit_workspace_bytes_ex(cfg, drop, 1), device=x.device, dtype=torch.uint8)
    feats = torch.empty(x.shape[0], m.num_tokens, m.embed_dim, device=x.device)
    if drop is None:
        check(h.mfvit_vit_forward(cfg, ptr(arena), ptr(m._shadow), ptr(x), ptr(ws), ptr(feats), stream()), "mfvit_vit_forward")
    else:
        check(h.mfvit_vit_forward_drop(cfg, drop, ptr(arena), ptr(m._shadow), ptr(x), ptr(ws), ptr(feats), stream()), "mfvit_vit_forward_drop")
    gflat, dimg = torch.zeros_like(arena), torch.empty_like(x)
    check(h.mfvit_vit_backward_ex(cfg, drop, ptr(arena), ptr(m._shadow), ptr(ws), ptr(r), ptr(gflat), ptr(dimg), m.depth, -1, stream()),
          "mfvit_vit_backward_ex")
    torch.cuda.synchronize()
    return feats, gflat, dimg


@pytest.mark.parametrize("precision", CHAIN_PRECISIONS)
def test_features3d_gives_the_bits_of_the_whole_stack_entry_points(precision):
    m, x = _chain_case(precision, 7101)
    r = rng_tensor(7103, (2, 17, 384)).to("cuda:0")
    got = _through_model(m, x, r)
    want = _whole_stack_calls(m, x, r, None)
    for name, a, b in zip(("features", "gradient arena", "d img"), got, want):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0 and torch.equal(a, b), name


def test_features3d_with_dropout_gives_the_bits_of_the_whole_stack_entry_points():
    m, x = _chain_case("bf16x3", 7111, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2)
    r = rng_tensor(7113, (2, 17, 384)).to("cuda:0")
    got = _through_model(m, x, r)
    want = _whole_stack_calls(m, x, r, m._last_drop)    # (the masks of the model's forward: the same rates and seed)
    for name, a, b in zip(("features", "gradient arena", "d img"), got, want):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0 and torch.equal(a, b), name
    with torch.no_grad():                               # (the masks do act: the evaluation forward differs)
        assert not torch.equal(m.eval().features3D(x), got[0])


@pytest.mark.parametrize("precision", CHAIN_PRECISIONS)
def test_kept_patches_give_the_bits_of_the_given_x0_entry_points(precision):
    from mfvit import _lib
    from mfvit._lib import check, lib, ptr, stream
    m, x = _chain_case(precision, 7121)
    B, K, D = 2, 8, 384
    idx = torch.stack([torch.randperm(16, generator=torch.Generator().manual_seed(7123 + b))[:K] for b in range(B)]).to("cuda:0")
    r = rng_tensor(7124, (B, 1 + K, D)).to("cuda:0")
    got = _through_model(m, x, r, keep_indices=idx)
    m.check_keep_error()
    # mfvit_patch_keep_embed + mfvit_vit_forward_x0 + mfvit_vit_backward_x0 + mfvit_patch_keep_embed_bwd on fresh buffers
    cfg = m._cfg(x, True)
    m._ensure_shadow(cfg)
    h, arena, dev = lib(), m.flat_parameters(), x.device
    pk = _lib.PatchKeepCfg(cfg.dtype, B, 64, 64, K, D)
    fws = torch.empty(h.mfvit_patch_keep_workspace_bytes(pk, 1), device=dev, dtype=torch.uint8)
    ws = torch.empty(h.mfvit_vit_workspace_bytes_x0(cfg, None, 1 + K), device=dev, dtype=torch.uint8)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    x0, feats, dx0 = (torch.empty(B, 1 + K, D, device=dev) for _ in range(3))
    gflat, dimg = torch.zeros_like(arena), torch.empty_like(x)
    names = ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias")
    p_cls, p_pos, p_w, p_b = (arena.data_ptr() + 4 * m.arena_slice(n)[0] for n in names)
    g_cls, _, g_w, g_b = (gflat.data_ptr() + 4 * m.arena_slice(n)[0] for n in names)
    check(h.mfvit_patch_keep_embed(pk, ptr(x), ptr(idx), p_cls, p_pos, p_w, p_b, ptr(fws), 1, ptr(x0), ptr(err), stream()), "mfvit_patch_keep_embed")
    check(h.mfvit_vit_forward_x0(cfg, None, 1 + K, ptr(arena), ptr(m._shadow), ptr(x0), ptr(ws), ptr(feats), stream()), "mfvit_vit_forward_x0")
    check(h.mfvit_vit_backward_x0(cfg, None, 1 + K, ptr(arena), ptr(m._shadow), ptr(ws), ptr(r), ptr(gflat), ptr(dx0), m.depth, -1, stream()),
          "mfvit_vit_backward_x0")
    check(h.mfvit_patch_keep_embed_bwd(pk, ptr(idx), ptr(fws), ptr(dx0), g_cls, g_w, g_b, ptr(dimg), ptr(err), stream()), "mfvit_patch_keep_embed_bwd")
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and got[0].shape == (B, 1 + K, D)
    for name, a, b in zip(("features", "gradient arena", "d img"), got, (feats, gflat, dimg)):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0 and torch.equal(a, b), name


@pytest.mark.parametrize("precision", CHAIN_PRECISIONS)
def test_the_stage_hook_sees_every_group_and_leaves_the_bits(precision):
    m, x = _chain_case(precision, 7131)
    r = rng_tensor(7133, (2, 17, 384)).to("cuda:0")
    want = _through_model(m, x, r)
    seen = []
    m._grad_bucket_layers = 1
    m._grad_stage_hook = lambda vit, hi, lo, gflat: seen.append((vit is m, hi, lo, gflat is not None))
    got = _through_model(m, x, r)
    del m._grad_stage_hook
    assert seen == [(True, 2, 1, True), (True, 0, -1, True)]        # depth 2: (depth, depth - 1), (depth - 2, -1)
    for name, a, b in zip(("features", "gradient arena", "d img"), got, want):
        assert torch.equal(a, b), name
