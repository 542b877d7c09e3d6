"""Attention maps and attention rollout of the ViT encoders on the GPU (include/mfvit.h, mfvit_vit_forward_attn; csrc/attention_maps.hip).

Reference: the block loop of oracle.ref_vit restated in float64 on the CPU, keeping every block's softmax probabilities.  Gates: measured on
an MI355X, then fixed at >= 2 x the measured error and never looser than the TOL of tests/test_input_grad_gpu.py."""
import ctypes

import pytest
import torch

from conftest import rng_tensor
from oracle import ref_vit

DEV = "cuda:0"
# largest error measured on one MI355X over the maps, fusions, cls rows and rollouts of CASES: fp32 3.7e-6, bf16x3 7.7e-5, fp16 2.4e-3,
# bf16 1.8e-2 (the TOL of tests/test_input_grad_gpu.py: 1e-5, 1e-3, 1e-2, 4e-2)
TOL = {"fp32": 1e-5, "bf16x3": 2e-4, "fp16": 5e-3, "bf16": 4e-2}
FUSIONS = ("mean", "max", "min")
# (arch, img_size, precision): every storage format of the qkv tensor (mfvit_attention_qkv_dtype)
CASES = [("vit_small", 224, "fp32"), ("vit_small", 224, "bf16"), ("vit_small", 224, "fp16"), ("vit_small", 224, "bf16x3"),
         ("vit_small", 384, "bf16x3"), ("vit_base", 224, "bf16x3"), ("vit_small", (224, 320), "bf16x3")]


def rel_err(got, ref):
    ref, got = ref.detach().double().cpu(), got.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def build(arch="vit_small", depth=12, precision="bf16x3", seed=7, img_size=224, **kw):
    import vits
    m = getattr(vits, arch)(num_classes=3, depth=depth, precision=precision, img_size=img_size, **kw)
    sd = ref_vit.seeded_params(seed, arch=arch, num_classes=3, depth=depth)
    sd["pos_embed"] = m.pos_embed.detach().clone()      # (the fixed sin-cos table of the model's own grid: non-square images too)
    m.load_state_dict(sd)
    return m.to(DEV), sd


def ref_probs(sd, img, heads=12):
    """float64 softmax probabilities (B, H, T, T) of every block: oracle.ref_vit's patch_embed / layer_norm / block, and mhsa's qkv / softmax."""
    p = {k: v.double() for k, v in sd.items()}
    x = ref_vit.patch_embed(p, img.double())
    x = torch.cat([p["cls_token"].expand(x.shape[0], -1, -1), x], dim=1) + p["pos_embed"]
    out = []
    for i in range(ref_vit.depth_of(p)):
        pre = f"blocks.{i}."
        y = ref_vit.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], ref_vit.LN_EPS)
        B, T, D = y.shape
        d = D // heads
        qkv = (y @ p[pre + "attn.qkv.weight"].t() + p[pre + "attn.qkv.bias"]).reshape(B, T, 3, heads, d).permute(2, 0, 3, 1, 4)
        out.append((qkv[0] @ qkv[1].transpose(-2, -1) * d ** -0.5).softmax(dim=-1))
        x = ref_vit.block(p, i, x, heads)
    return out


def fuse(P, how):
    return {"mean": lambda t: t.mean(dim=1), "max": lambda t: t.amax(dim=1), "min": lambda t: t.amin(dim=1)}[how](P)


def ref_rollout(probs, how):
    R = None
    for P in probs:
        F = fuse(P, how)
        A = 0.5 * F + 0.5 * torch.eye(F.shape[-1], dtype=F.dtype)
        A = A / A.sum(dim=-1, keepdim=True)
        R = A if R is None else A @ R
    return R[:, 0, 1:]


def qkv_dtype(precision, arch, img_size):
    from mfvit import _lib
    h, w = (img_size, img_size) if isinstance(img_size, int) else img_size
    hd = {"vit_small": 32, "vit_base": 64}[arch]
    return _lib.lib().mfvit_attention_qkv_dtype(_lib.dtype_code(precision), (h // 16) * (w // 16) + 1, hd)


@pytest.mark.gpu
def test_cases_reach_every_qkv_storage_format():
    from mfvit import _lib
    assert {qkv_dtype(p, a, s) for a, s, p in CASES} == {_lib.F32, _lib.BF16, _lib.F16, _lib.BF16X3, _lib.X3F16}


# ------------------------------------------------------------------------------------------------ 1 + 2. parity and row sums, every format
@pytest.mark.gpu
@pytest.mark.parametrize("arch,img_size,precision", CASES)
def test_maps_and_rollout_match_float64(arch, img_size, precision):
    B = 2
    m, sd = build(arch=arch, precision=precision, img_size=img_size)
    h, w = m.img_size
    img = rng_tensor(61, (B, 3, h, w))
    x = img.to(DEV)
    ref = ref_probs(sd, img)
    gate = TOL[precision]
    tag = f"[{arch} {img_size} {precision} qkv dtype {qkv_dtype(precision, arch, img_size)}]"
    maps = m.get_attention_maps(x)
    assert len(maps) == m.depth
    errs = [rel_err(g, r) for g, r in zip(maps, ref)]
    sums = max(float((g.double().sum(dim=-1) - 1).abs().max()) for g in maps)
    print(f"{tag} per head: max rel err {max(errs):.2e}, row sums |s - 1| {sums:.2e}")
    assert maps[0].shape == (B, 12, m.num_tokens, m.num_tokens) and maps[0].dtype == torch.float32
    assert max(errs) < gate, errs
    assert sums < 1e-4, sums
    cls = m.get_attention_maps(x, cls_only=True)
    e = max(rel_err(g, r[:, :, 0]) for g, r in zip(cls, ref))
    print(f"{tag} cls_only: {e:.2e}")
    assert cls[0].shape == (B, 12, m.num_tokens) and e < gate
    for how in FUSIONS:
        fm = m.get_attention_maps(x, head_fusion=how)
        e = max(rel_err(g, fuse(r, how)) for g, r in zip(fm, ref))
        ro = m.attention_rollout(x, head_fusion=how)
        rr = ref_rollout(ref, how)
        er = rel_err(ro.reshape(B, -1), rr)
        print(f"{tag} {how}: maps {e:.2e}, rollout {er:.2e}")
        assert fm[0].shape == (B, m.num_tokens, m.num_tokens) and e < gate
        assert ro.shape == (B, h // 16, w // 16) and er < gate


# ------------------------------------------------------------------------------------------------ 3. internal consistency
@pytest.mark.gpu
@pytest.mark.parametrize("arch,precision", [("vit_small", "bf16x3"), ("vit_small", "fp32"), ("vit_base", "bf16x3")])
def test_internal_consistency(arch, precision):
    m, _ = build(arch=arch, precision=precision, depth=4)
    x = rng_tensor(62, (3, 3, 224, 224)).to(DEV)
    last = m.get_last_selfattention(x)
    assert torch.equal(last, m.get_attention_maps(x, blocks=[m.depth - 1])[0])
    assert torch.equal(last, m.get_attention_maps(x, blocks=[-1])[0])
    full = m.get_attention_maps(x)
    again = m.get_attention_maps(x)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    assert torch.equal(last, full[-1])
    sel = m.get_attention_maps(x, blocks=[2, 0])
    assert torch.equal(sel[0], full[0]) and torch.equal(sel[1], full[2])
    for f, P in zip(m.get_attention_maps(x, head_fusion="max"), full):
        assert torch.equal(f, P.amax(dim=1))
    for f, P in zip(m.get_attention_maps(x, head_fusion="min"), full):
        assert torch.equal(f, P.amin(dim=1))
    for f, P in zip(m.get_attention_maps(x, head_fusion="mean"), full):
        assert float((f - P.mean(dim=1)).abs().max()) < 1e-6
    for c, P in zip(m.get_attention_maps(x, cls_only=True), full):
        assert float((c - P[:, :, 0]).abs().max()) < 1e-6
    for c, P in zip(m.get_attention_maps(x, head_fusion="max", cls_only=True), full):
        assert float((c - P.amax(dim=1)[:, 0]).abs().max()) < 1e-6
    r1, r2 = m.attention_rollout(x), m.attention_rollout(x)
    assert torch.equal(r1, r2)


# ------------------------------------------------------------------------------------------------ 4. no effect on the forward
@pytest.mark.gpu
def test_forward_attn_features_are_bit_identical_and_model_output_unchanged():
    from mfvit import _lib
    m, _ = build(depth=3)
    m.eval()
    x = rng_tensor(63, (2, 3, 224, 224)).to(DEV)
    with torch.no_grad():
        before = m(x).clone()
    h = _lib.lib()
    img = x.contiguous()
    cfg = m._cfg(img, False)
    m._ensure_shadow(cfg)
    T = m.num_tokens
    f0 = torch.empty(2, T, 384, device=DEV)
    f1 = torch.empty_like(f0)
    ws = torch.empty(h.mfvit_vit_workspace_bytes(cfg), device=DEV, dtype=torch.uint8)
    maps = torch.empty(2 * 2 * T * T, device=DEV)
    roll = torch.empty(2, T - 1, device=DEV)
    req = _lib.VitAttnReq(0b101, 1, 0, maps.data_ptr(), roll.data_ptr(), None)
    scratch = torch.empty(h.mfvit_vit_attn_scratch_bytes(cfg, req), device=DEV, dtype=torch.uint8)
    req.scratch = scratch.data_ptr()
    s = _lib.stream()
    assert h.mfvit_vit_forward(cfg, m._arena.data_ptr(), m._shadow.data_ptr(), img.data_ptr(), ws.data_ptr(), f0.data_ptr(), s) == 0
    assert h.mfvit_vit_forward_attn(cfg, ctypes.byref(req), m._arena.data_ptr(), m._shadow.data_ptr(), img.data_ptr(), ws.data_ptr(),
                                    f1.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(f0, f1)
    mean = m.get_attention_maps(x, blocks=[0, 2], head_fusion="mean")
    assert torch.equal(maps.view(2, 2, T, T)[0], mean[0]) and torch.equal(maps.view(2, 2, T, T)[1], mean[1])
    assert torch.equal(roll.view(2, 14, 14), m.attention_rollout(x))
    m.get_last_selfattention(x)
    with torch.no_grad():
        after = m(x)
    assert torch.equal(before, after)


# ------------------------------------------------------------------------------------------------ 5. evaluation semantics
@pytest.mark.gpu
def test_training_mode_gives_evaluation_maps_and_draws_no_seed():
    m, _ = build(depth=3, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1)
    x = rng_tensor(64, (2, 3, 224, 224)).to(DEV).requires_grad_(True)
    m.train()
    rng = torch.get_rng_state()
    cache = m._feat_cache
    got = (m.get_attention_maps(x), m.get_attention_maps(x, head_fusion="max", cls_only=True), m.get_last_selfattention(x),
           m.attention_rollout(x, head_fusion="min"))
    assert torch.equal(torch.get_rng_state(), rng)
    assert m.training and m._feat_cache is cache
    flat = got[0] + got[1] + [got[2], got[3]]
    assert not any(t.requires_grad for t in flat)
    m.eval()
    ref = (m.get_attention_maps(x), m.get_attention_maps(x, head_fusion="max", cls_only=True), m.get_last_selfattention(x),
           m.attention_rollout(x, head_fusion="min"))
    assert all(torch.equal(a, b) for a, b in zip(flat, ref[0] + ref[1] + [ref[2], ref[3]]))


# ------------------------------------------------------------------------------------------------ 6. no per-head maps on the rollout path
@pytest.mark.gpu
def test_rollout_memory_holds_no_per_head_maps():
    B = 128
    m, _ = build()
    m.eval()
    x = rng_tensor(65, (B, 3, 224, 224)).to(DEV)
    T = m.num_tokens

    def rise(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return peak

    def plain():
        with torch.no_grad():
            return m.features3D(x)
    plain()                                               # (warms the workspace pool)
    r_fwd = rise(plain)
    r_roll = rise(lambda: m.attention_rollout(x))
    budget = 1.25 * m.depth * B * T * T * 4
    print(f"peak rise: no-grad forward {r_fwd / 2**20:.1f} MiB, rollout {r_roll / 2**20:.1f} MiB (budget above the forward "
          f"{budget / 2**20:.1f} MiB)")
    assert r_roll - r_fwd <= budget
