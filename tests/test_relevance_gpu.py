"""Class-specific attention relevance of the ViT encoders on the GPU (include/mfvit.h, mfvit_vit_backward_rel; csrc/attention_maps.hip):
Chefer, Gur & Wolf 2021, the self-attention rule, A_l = mean_h max(0, P_h o d y_t / d P_h) and the cls row of R = (I + A_{L-1}) ... (I + A_0).

Reference: the block loop of oracle.ref_vit restated in float64 on the CPU with every block's softmax probabilities kept (retain_grad), the
class score differentiated by torch autograd.  Gates: measured on an MI355X, then fixed at >= 2 x the measured error and never looser than the
TOL of tests/test_input_grad_gpu.py."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rng_tensor
from oracle import ref_fusion, ref_vit

DEV = "cuda:0"
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
# the TOL of tests/test_input_grad_gpu.py: the ceiling of every gate below
TOL = {"fp32": 1e-5, "bf16x3": 1e-3, "fp16": 1e-2, "bf16": 4e-2}
# largest error measured on one MI355X over every block's map and the relevance of CASES: fp32 3.8e-6, bf16x3 4.7e-4, fp16 1.5e-3, bf16 1.3e-2;
# Fus_CrossViT (bf16x3) 3.4e-4
GATE = {"fp32": 1e-5, "bf16x3": 1e-3, "fp16": 4e-3, "bf16": 3e-2}
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


def ref_features(p, img, heads=12):
    """float64 features3D with every block's probabilities P (B, H, T, T) kept for their gradient: oracle.ref_vit's patch_embed / layer_norm /
    gelu_erf, and mhsa / block restated."""
    x = ref_vit.patch_embed(p, img)
    x = torch.cat([p["cls_token"].expand(x.shape[0], -1, -1), x], dim=1) + p["pos_embed"]
    probs = []
    for i in range(ref_vit.depth_of(p)):
        pre = f"blocks.{i}."
        y = ref_vit.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], ref_vit.LN_EPS)
        B, T, D = y.shape
        d = D // heads
        qkv = (y @ p[pre + "attn.qkv.weight"].t() + p[pre + "attn.qkv.bias"]).reshape(B, T, 3, heads, d).permute(2, 0, 3, 1, 4)
        P = (qkv[0] @ qkv[1].transpose(-2, -1) * d ** -0.5).softmax(dim=-1)
        P.retain_grad()
        probs.append(P)
        o = (P @ qkv[2]).transpose(1, 2).reshape(B, T, D)
        x = x + o @ p[pre + "attn.proj.weight"].t() + p[pre + "attn.proj.bias"]
        y = ref_vit.layer_norm(x, p[pre + "norm2.weight"], p[pre + "norm2.bias"], ref_vit.LN_EPS)
        h = ref_vit.gelu_erf(y @ p[pre + "mlp.fc1.weight"].t() + p[pre + "mlp.fc1.bias"])
        x = x + h @ p[pre + "mlp.fc2.weight"].t() + p[pre + "mlp.fc2.bias"]
    return ref_vit.layer_norm(x, p["norm.weight"], p["norm.bias"], ref_vit.LN_EPS), probs


def chefer(probs):
    """A_l of every block and the cls row of R (Chefer's R = I; R += A_l R), after the score's backward."""
    A = [(P * P.grad).clamp(min=0).mean(dim=1).detach() for P in probs]
    T = A[0].shape[-1]
    R = torch.eye(T, dtype=A[0].dtype).expand_as(A[0]).clone()
    for a in A:
        R = R + a @ R
    return A, R[:, 0, 1:]


def ref_relevance(sd, img, target, heads=12):
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    f, probs = ref_features(p, img.double(), heads)
    ref_vit.head_linear(p, f[:, 0]).gather(1, target.view(-1, 1)).sum().backward()
    return chefer(probs)


def qkv_dtype(precision, arch, img_size):
    from mfvit import _lib
    h, w = (img_size, img_size) if isinstance(img_size, int) else img_size
    hd = {"vit_small": 32, "vit_base": 64}[arch]
    return _lib.lib().mfvit_attention_qkv_dtype(_lib.dtype_code(precision), (h // 16) * (w // 16) + 1, hd)


@pytest.mark.gpu
def test_cases_reach_every_qkv_storage_format():
    from mfvit import _lib
    assert {qkv_dtype(p, a, s) for a, s, p in CASES} == {_lib.F32, _lib.BF16, _lib.F16, _lib.BF16X3, _lib.X3F16}


# ------------------------------------------------------------------------------------------------ 1. parity with float64, every format
@pytest.mark.gpu
@pytest.mark.parametrize("arch,img_size,precision", CASES)
def test_relevance_maps_and_relevance_match_float64(arch, img_size, precision):
    B = 2
    # vit_base runs 4 blocks, as the vit_base case of tests/test_input_grad_gpu.py: at depth 12 its block-0 map measured 8.9e-4 - the error of
    # eleven blocks of bf16x3 data-gradient chain in front of it, the image gradient's error class - which leaves no 2 x margin under TOL
    m, sd = build(arch=arch, precision=precision, img_size=img_size, depth=4 if arch == "vit_base" else 12)
    h, w = m.img_size
    img = rng_tensor(71, (B, 3, h, w))
    x = img.to(DEV)
    t = torch.tensor([2, 0])
    A_ref, r_ref = ref_relevance(sd, img, t)
    gate = GATE[precision]
    assert gate <= TOL[precision]
    maps = m.get_relevance_maps(x, target=t.to(DEV))
    rel = m.attention_relevance(x, target=t.to(DEV))
    assert len(maps) == m.depth and maps[0].shape == (B, m.num_tokens, m.num_tokens) and maps[0].dtype == torch.float32
    assert rel.shape == (B, h // 16, w // 16) and rel.dtype == torch.float32
    errs = [rel_err(g, r) for g, r in zip(maps, A_ref)]
    er = rel_err(rel.reshape(B, -1), r_ref)
    print(f"[{arch} {img_size} {precision} qkv dtype {qkv_dtype(precision, arch, img_size)}] maps: max rel err {max(errs):.2e} "
          f"(per block {', '.join(f'{e:.1e}' for e in errs)}), relevance {er:.2e}")
    assert max(errs) < gate, errs
    assert er < gate, er


# ------------------------------------------------------------------------------------------------ 1b. the relevance is the chain of the maps
# The update kernel against the maps kernel's own output: v = e_0, v <- v + v A_l for l = L-1 .. 0 in float64 over the GPU's f32 maps.  This
# gates the full-depth vit_base chain too, whose float64 parity is printed but not gated (its block-0 map measured 8.9e-4 against the reference,
# the error of the bf16x3 data-gradient chain in front of it: no 2 x margin under TOL).  Largest error measured on one MI355X: 8.4e-7 (vit_small, depth 12; vit_base 2.5e-7).
CHAIN_GATE = 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("arch,depth", [("vit_base", 12), ("vit_small", 12), ("vit_small", 1)])
def test_relevance_is_the_cls_row_chain_of_the_maps(arch, depth):
    B = 2
    m, sd = build(arch=arch, depth=depth)
    img = rng_tensor(80, (B, 3, 224, 224))
    x = img.to(DEV)
    t = torch.tensor([0, 1])
    maps, rel = m._relevance(x, t, list(range(depth)), True)
    v = torch.zeros(B, m.num_tokens, dtype=torch.float64)
    v[:, 0] = 1
    for a in reversed(maps):
        v = v + torch.einsum("bi,bij->bj", v, a.double().cpu())
    e = rel_err(rel, v[:, 1:])
    msg = f"[{arch} depth {depth}] relevance vs the chain of its own maps {e:.2e}"
    if arch == "vit_base":
        A_ref, r_ref = ref_relevance(sd, img, t)
        msg += f"; against float64 (not gated): maps {max(rel_err(g, r) for g, r in zip(maps, A_ref)):.2e}, relevance {rel_err(rel, r_ref):.2e}"
    print(msg)
    assert e < CHAIN_GATE, e


@pytest.mark.gpu
def test_maps_only_request_runs_on_the_documented_256_bytes_of_scratch():
    from mfvit import _lib
    m, _ = build(depth=3)
    x = rng_tensor(81, (2, 3, 224, 224)).to(DEV)
    t = torch.tensor([2, 1], device=DEV)
    want = m.get_relevance_maps(x, target=t)
    cfg, ws, feats = m._rel_forward(x)
    try:
        f = feats.detach().requires_grad_(True)
        with torch.enable_grad():
            (df,) = torch.autograd.grad(m.forward_head(f).gather(1, t.view(-1, 1)).sum(), f)
        T = m.num_tokens
        maps = torch.empty(3, 2, T, T, device=DEV)
        req = _lib.VitRelReq(0b111, maps.data_ptr(), None, None)
        assert _lib.lib().mfvit_vit_rel_scratch_bytes(cfg, req) == 256
        scratch = torch.empty(256, device=DEV, dtype=torch.uint8)
        req.scratch = scratch.data_ptr()
        assert _lib.lib().mfvit_vit_backward_rel(cfg, req, m._arena.data_ptr(), m._shadow.data_ptr(), ws.data_ptr(),
                                                 df.contiguous().data_ptr(), _lib.stream()) == 0
        torch.cuda.synchronize()
    finally:
        m._release_ws(ws)
    assert all(torch.equal(maps[i], want[i]) for i in range(3))


# ------------------------------------------------------------------------------------------------ 2. targets
@pytest.mark.gpu
def test_targets():
    m, _ = build(depth=4)
    m.eval()
    x = rng_tensor(72, (3, 3, 224, 224)).to(DEV)
    with torch.no_grad():
        am = m(x).argmax(dim=1)
    assert torch.equal(m.attention_relevance(x), m.attention_relevance(x, target=am))
    assert all(torch.equal(a, b) for a, b in zip(m.get_relevance_maps(x), m.get_relevance_maps(x, target=am)))
    for c in range(3):
        tc = torch.full((3,), c, dtype=torch.int64, device=DEV)
        assert torch.equal(m.attention_relevance(x, target=c), m.attention_relevance(x, target=tc))
        assert torch.equal(m.attention_relevance(x, target=c), m.attention_relevance(x, target=tc.int()))
    r0, r1 = m.attention_relevance(x, target=0), m.attention_relevance(x, target=1)
    assert not torch.equal(r0, r1)
    assert float((r0 - r1).abs().max()) > 1e-3 * float(r0.abs().max())
    mixed = m.attention_relevance(x, target=torch.tensor([0, 1, 0]))
    assert torch.equal(mixed[0], r0[0]) and torch.equal(mixed[1], r1[1]) and torch.equal(mixed[2], r0[2])


# ------------------------------------------------------------------------------------------------ 3. same bits
@pytest.mark.gpu
@pytest.mark.parametrize("arch,precision", [("vit_small", "bf16x3"), ("vit_small", "fp32"), ("vit_base", "bf16x3")])
def test_same_bits(arch, precision):
    m, _ = build(arch=arch, precision=precision, depth=4)
    x = rng_tensor(73, (3, 3, 224, 224)).to(DEV)
    t = torch.tensor([1, 2, 0], device=DEV)
    r1, r2 = m.attention_relevance(x, target=t), m.attention_relevance(x, target=t)
    assert torch.equal(r1, r2)
    full = m.get_relevance_maps(x, target=t)
    again = m.get_relevance_maps(x, target=t)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    both, r3 = m._relevance(x, t, list(range(m.depth)), True)           # maps and relevance in one call
    assert torch.equal(r3.view_as(r1), r1)
    assert all(torch.equal(a, b) for a, b in zip(both, full))
    for l in range(m.depth):
        assert torch.equal(m.get_relevance_maps(x, target=t, blocks=[l])[0], full[l])
    assert torch.equal(m.get_relevance_maps(x, target=t, blocks=[-1])[0], full[-1])
    sel = m.get_relevance_maps(x, target=t, blocks=[2, 0])
    assert torch.equal(sel[0], full[0]) and torch.equal(sel[1], full[2])
    assert all(bool((a >= 0).all()) and bool(torch.isfinite(a).all()) for a in full)


@pytest.mark.gpu
def test_same_bits_at_batch_128():
    m, _ = build()
    x = rng_tensor(74, (128, 3, 224, 224)).to(DEV)
    r1, r2 = m.attention_relevance(x), m.attention_relevance(x)
    assert torch.equal(r1, r2) and float(r1.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. no side effects
@pytest.mark.gpu
def test_no_gradients_no_arena_no_state_change_in_training_mode_with_dropout():
    m, _ = build(depth=3, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1)
    x = rng_tensor(75, (2, 3, 224, 224)).to(DEV)
    m.train()
    F.cross_entropy(m(x), torch.tensor([0, 1], device=DEV)).backward()     # a gradient arena exists
    m.zero_grad(set_to_none=True)
    arena = m._grad_arena
    snap = arena.clone()
    m.eval()
    with torch.no_grad():
        m.features3D(x)                                                     # (a feature cache entry: evaluation forwards keep one)
    m.train()
    cache = m._feat_cache
    assert cache is not None
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    t = torch.tensor([2, 1], device=DEV)
    got = (m.attention_relevance(x, target=t), m.get_relevance_maps(x, target=t), m.attention_relevance(x))
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())
    assert m._grad_arena is arena and torch.equal(arena, snap)
    assert m._feat_cache is cache and m.training
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    assert not got[0].requires_grad and not any(a.requires_grad for a in got[1])
    m.eval()                                                                # training mode gave the evaluation relevance
    assert torch.equal(got[0], m.attention_relevance(x, target=t))
    assert all(torch.equal(a, b) for a, b in zip(got[1], m.get_relevance_maps(x, target=t)))


@pytest.mark.gpu
def test_moco_base_encoder_batchnorm_head_statistics_do_not_move():
    import types
    from functools import partial
    import vits
    import moco.builder_vit_mocov3structure_mocov2loss as bld
    torch.manual_seed(0)
    moco = bld.MoCo_ViT(partial(vits.vit_small, depth=3), types.SimpleNamespace(arch="vit_small"), 256, 512, 0.2).to(DEV)
    m = moco.base_encoder                                                   # head: MoCo's projector MLP with BatchNorm (BLD:62-78)
    m.train()
    x = rng_tensor(76, (8, 3, 224, 224)).to(DEV)
    m(x).sum().backward()                                                   # (moves the statistics once: they are not at their defaults)
    m.zero_grad(set_to_none=True)
    bufs = {k: v.clone() for k, v in m.head.state_dict().items()}
    rel = m.attention_relevance(x)
    rel5 = m.attention_relevance(x, target=5)
    assert rel.shape == (8, 14, 14) and torch.isfinite(rel).all() and torch.isfinite(rel5).all()
    assert not torch.equal(rel, rel5)
    assert all(torch.equal(v, m.head.state_dict()[k]) for k, v in bufs.items())
    assert all(mod.training for mod in m.head.modules())
    assert all(p.grad is None for p in m.parameters())
    with pytest.raises(ValueError):
        m.attention_relevance(x, target=256)
    assert all(mod.training for mod in m.head.modules())


@pytest.mark.gpu
def test_training_step_after_a_relevance_call_is_bit_identical_to_a_fresh_models():
    x = rng_tensor(77, (4, 3, 224, 224)).to(DEV)
    y = torch.tensor([0, 1, 2, 0], device=DEV)
    runs = []
    for call in (True, False):
        m, _ = build(depth=4)
        m.train()
        if call:
            m.attention_relevance(x)
            m.get_relevance_maps(x, target=1, blocks=[0, 3])
        logits = m(x)
        F.cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), [p.grad.clone() for p in m.parameters() if p.requires_grad]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert len(runs[0][1]) == len(runs[1][1]) > 50
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ------------------------------------------------------------------------------------------------ 5. Fus_CrossViT
def _ca():
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    depth = 3
    vit_p = [ref_vit.seeded_params(17 + i, num_classes=3, depth=depth) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(19)
    backs = []
    for p in vit_p:
        b = vits.vit_small(num_classes=3, depth=depth)
        b.load_state_dict(p)
        backs.append(b.to(DEV))
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    return model.to(DEV), backs, vit_p, fus_p


@pytest.mark.gpu
@pytest.mark.parametrize("heads", ["fused", "plain"])
@pytest.mark.parametrize("two_streams", [True, False])
def test_fus_crossvit_relevance_matches_float64(two_streams, heads):
    # attention_relevance runs the two encoders one after the other on the caller's stream whatever _two_streams says; what the setting changes
    # is the launch-geometry hint (mfvit_vit_cfg.stream_share) a forward leaves on the encoders, and the relevance after such a forward is checked
    model, backs, vit_p, fus_p = _ca()
    model._two_streams = two_streams
    if heads == "plain":
        model._plain_head = lambda vit: None                 # the fusion without heads + each backbone's own forward_head
    B = 2
    xc, xe = rng_tensor(78, (B, 3, 224, 224)), rng_tensor(79, (B, 3, 224, 224))
    t = torch.tensor([1, 2])
    with torch.no_grad():
        fused, x_c, x_e = model(backs[0], backs[1], xc.to(DEV), xe.to(DEV))
    assert all(b._stream_share == (2 if two_streams else 1) for b in backs)
    rc, re_ = model.attention_relevance(backs[0], backs[1], xc.to(DEV), xe.to(DEV), target=t.to(DEV))
    assert rc.shape == re_.shape == (B, 14, 14)
    fp = {k: v.double().requires_grad_(True) for k, v in fus_p.items()}
    vp = [{k: v.double().requires_grad_(True) for k, v in p.items()} for p in vit_p]
    fc, pc = ref_features(vp[0], xc.double())
    fe, pe = ref_features(vp[1], xe.double())
    out = ref_fusion.fus_from_features(fp, fc, fe) + ref_vit.head_linear(vp[0], fc[:, 0]) + ref_vit.head_linear(vp[1], fe[:, 0])
    out.gather(1, t.view(-1, 1)).sum().backward()
    (_, r_c), (_, r_e) = chefer(pc), chefer(pe)
    ec, ee = rel_err(rc.reshape(B, -1), r_c), rel_err(re_.reshape(B, -1), r_e)
    print(f"[CA two={two_streams} heads={heads}] relevance cxr {ec:.2e}, enh {ee:.2e}")
    assert ec < GATE["bf16x3"] and ee < GATE["bf16x3"], (ec, ee)
    assert all(p.grad is None for b in backs for p in b.parameters())
    assert all(p.grad is None for p in model.parameters())
    # target None: the argmax of the summed output
    am = (fused + x_c + x_e).argmax(dim=1)
    a = model.attention_relevance(backs[0], backs[1], xc.to(DEV), xe.to(DEV))
    b = model.attention_relevance(backs[0], backs[1], xc.to(DEV), xe.to(DEV), target=am)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
