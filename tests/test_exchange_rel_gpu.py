"""Exchange attention maps, gradient-weighted exchange maps and cross-stream relevance of Fus_CrossViT on the GPU (include/mfvit.h:
mfvit_fusion_ex_attention, mfvit_fusion_ex_grad_attention, mfvit_bimodal_relevance; csrc/fusion.hip, csrc/fusion_maps.hip).

Reference: tests/exchange_rel_ref.py, float64 on the CPU.  Checks 1 - 3 take the GPU's own f32 inputs (features, or synthetic maps), so they see
the f32 kernels alone; check 4 runs the whole float64 model.

Shapes (vit_small unless said; every encoder accepted every size):
  a  224 x 224, T = 197 (no multiple of 32 or 64), B = 2, exchange heads 3, encoder depth 3
  b  64 x 128,  T = 33 (one past a 32-wide tile),  B = 3, exchange heads 6 (two head chunks), encoder depth 2
  c  32 x 32,   T = 5 (fewer rows than waves),     B = 2, exchange heads 12 (four head chunks), encoder depth 2
  d  vit_base (width 768), 224 x 224, B = 2, exchange heads 3, encoder depth 2
and for the chain kernel alone also T = 1100 (more than 1024 tokens: several columns per thread, no row groups).

Gates: MEASURED holds the largest relative max-norm error of each check on one MI355X; every gate is >= 2 x that and never looser than the
project's ceilings (1e-5 for the f32 kernels on given inputs - the fp32 TOL / CHAIN_GATE of tests/test_relevance_gpu.py; 1e-3 = TOL["bf16x3"]
end to end)."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as F

import exchange_rel_ref as R
from conftest import rng_tensor
from oracle import ref_vit

DEV = "cuda:0"
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
CEIL_F32, CEIL_X3 = 1e-5, 1e-3
# largest error measured on one MI355X over every case of each check: attention 1.49e-6 (case d, two exchange layers; |row sum - 1| 1.4e-7),
# abar 1.03e-6 (case a), chain 1.2e-6 (T = 1100; 2.3e-7 at T = 197), cross 2.3e-4 (case a, rel_ee; vit_base 2.2e-4)
MEASURED = {"attention": 1.49e-6, "abar": 1.03e-6, "chain": 1.2e-6, "cross": 2.3e-4}
GATE = {"attention": CEIL_F32, "abar": CEIL_F32, "chain": CEIL_F32, "cross": CEIL_X3}
assert all(GATE[k] >= 2 * MEASURED[k] for k in GATE)
CASES = {
    "a": dict(arch="vit_small", img=(224, 224), B=2, heads=3, depth=3),
    "b": dict(arch="vit_small", img=(64, 128), B=3, heads=6, depth=2),
    "c": dict(arch="vit_small", img=(32, 32), B=2, heads=12, depth=2),
    "d": dict(arch="vit_base", img=(224, 224), B=2, heads=3, depth=2),
}
ENC_HEADS = 12
_cache = {}


def seeded_state(module, seed):
    sd = {}
    for i, (k, v) in enumerate(module.state_dict().items()):
        if v.dim() == 2:
            sd[k] = rng_tensor(seed * 1000 + i, tuple(v.shape), 0.06)
        elif k.endswith("bias"):
            sd[k] = rng_tensor(seed * 1000 + i, tuple(v.shape), 0.05)
        else:
            sd[k] = 1.0 + rng_tensor(seed * 1000 + i, tuple(v.shape), 0.1)
    return sd


def _ca(case, L=1, pool="cls", fresh=False):
    """(model, backbones, backbone state dicts, fusion state dict, images, target) of a case; built once per (case, L, pool) unless fresh."""
    key = (case, L, pool)
    if not fresh and key in _cache:
        return _cache[key]
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    c = CASES[case]
    seed = 300 + 10 * sorted(CASES).index(case)
    backs, vit_p = [], []
    for i in range(2):
        b = getattr(vits, c["arch"])(num_classes=3, depth=c["depth"], img_size=c["img"])
        sd = ref_vit.seeded_params(seed + i, arch=c["arch"], num_classes=3, depth=c["depth"])
        sd["pos_embed"] = b.pos_embed.detach().clone()      # (the fixed sin-cos table of the model's own grid)
        b.load_state_dict(sd)
        backs.append(b.to(DEV).eval())
        vit_p.append(sd)
    D = backs[0].embed_dim
    model = fus.Fus_CrossViT(backs[0], backs[1], small_dim=D, large_dim=D, heads=c["heads"], cross_attn_depth=L, pool=pool)
    fus_p = seeded_state(model, seed + 2)
    model.load_state_dict(fus_p)
    model = model.to(DEV).eval()
    B, (h, w) = c["B"], c["img"]
    imgs = (rng_tensor(seed + 3, (B, 3, h, w)), rng_tensor(seed + 4, (B, 3, h, w)))
    target = torch.arange(B) % 3
    out = (model, backs, vit_p, fus_p, imgs, target)
    if not fresh:
        _cache[key] = out
    return out


def _gpu_features(backs, imgs):
    with torch.no_grad():
        return [b.features3D(x.to(DEV)).detach().double().cpu() for b, x in zip(backs, imgs)]


def _d(sd, grad=False):
    return {k: v.double().requires_grad_(grad) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ 1. the exchange's probabilities
@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_exchange_attention_matches_float64_on_the_gpus_features(case, L):
    model, backs, _, fus_p, imgs, _ = _ca(case, L)
    H, B = CASES[case]["heads"], CASES[case]["B"]
    T = backs[0].num_tokens
    xc, xe = imgs[0].to(DEV), imgs[1].to(DEV)
    fc, fe = _gpu_features(backs, imgs)
    with torch.no_grad():
        _, kept = R.fus_forward_probs(_d(fus_p), fc, fe, H, L)
    per_head = model.get_exchange_attention(backs[0], backs[1], xc, xe)
    assert len(per_head) == L
    errs, sums = [], []
    for l in range(L):
        for got, ref in zip(per_head[l], kept[l]):
            assert got.shape == (B, H, T) and got.dtype == torch.float32 and not got.requires_grad
            errs.append(R.rel_err(got, ref[:, :, 0]))
            sums.append(float((got.double().sum(dim=-1) - 1).abs().max()))
    fused_err = []
    for hf, red in (("mean", lambda a: a.mean(dim=1)), ("max", lambda a: a.max(dim=1).values), ("min", lambda a: a.min(dim=1).values)):
        fused = model.get_exchange_attention(backs[0], backs[1], xc, xe, head_fusion=hf)
        for l in range(L):
            for got, ref in zip(fused[l], kept[l]):
                assert got.shape == (B, T)
                fused_err.append(R.rel_err(got, red(ref[:, :, 0])))
            if hf == "max":
                assert all(bool((g.sum(dim=-1) > 1).all()) for g in fused[l])          # not renormalised
    print(f"[exchange attention {case} L={L}] per head {max(errs):.2e}, fused {max(fused_err):.2e}, |row sum - 1| {max(sums):.2e}")
    assert max(errs) < GATE["attention"] and max(fused_err) < GATE["attention"], (errs, fused_err)
    assert max(sums) < GATE["attention"], sums


@pytest.mark.gpu
def test_exchange_attention_with_mean_pooling():
    model, backs, _, fus_p, imgs, _ = _ca("b", 1, "mean")
    fc, fe = _gpu_features(backs, imgs)
    with torch.no_grad():
        _, kept = R.fus_forward_probs(_d(fus_p), fc, fe, CASES["b"]["heads"], 1, "mean")
    got = model.get_exchange_attention(backs[0], backs[1], imgs[0].to(DEV), imgs[1].to(DEV))
    e = max(R.rel_err(g, r[:, :, 0]) for g, r in zip(got[0], kept[0]))
    print(f"[exchange attention b pool=mean] {e:.2e}")
    assert e < GATE["attention"], e


# ------------------------------------------------------------------------------------------------ 2. the gradient-weighted exchange map
def _ref_abar(vit_p, fus_p, fc, fe, H, t):
    fp = _d(fus_p, True)
    vp = [_d(p) for p in vit_p]
    lc, le = fc.clone().requires_grad_(True), fe.clone().requires_grad_(True)
    fused, kept = R.fus_forward_probs(fp, lc, le, H)
    out = fused + ref_vit.head_linear(vp[0], lc[:, 0]) + ref_vit.head_linear(vp[1], le[:, 0])
    out.gather(1, t.view(-1, 1)).sum().backward()
    return R.abar_of(kept[0][0]), R.abar_of(kept[0][1]), out.detach()


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_exchange_relevance_matches_float64_on_the_gpus_features(case):
    model, backs, vit_p, fus_p, imgs, t = _ca(case)
    B, T = CASES[case]["B"], backs[0].num_tokens
    xc, xe = imgs[0].to(DEV), imgs[1].to(DEV)
    fc, fe = _gpu_features(backs, imgs)
    r_c, r_e, out = _ref_abar(vit_p, fus_p, fc, fe, CASES[case]["heads"], t)
    g_c, g_e = model.exchange_relevance(backs[0], backs[1], xc, xe, target=t.to(DEV))
    assert g_c.shape == g_e.shape == (B, T) and g_c.dtype == torch.float32 and not g_c.requires_grad
    assert bool((g_c >= 0).all()) and bool((g_e >= 0).all()) and float(r_c.max()) > 0 and float(r_e.max()) > 0
    ec, ee = R.rel_err(g_c, r_c), R.rel_err(g_e, r_e)
    print(f"[exchange relevance {case}] Abar cxr {ec:.2e}, enh {ee:.2e}")
    assert ec < GATE["abar"] and ee < GATE["abar"], (ec, ee)
    # target None: the argmax of the summed output; the plain-head route (each backbone's own forward_head) scores the same class
    am = out.argmax(dim=1)
    a = model.exchange_relevance(backs[0], backs[1], xc, xe)
    b = model.exchange_relevance(backs[0], backs[1], xc, xe, target=am.to(DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    model._plain_head = lambda vit: None
    try:
        p_c, p_e = model.exchange_relevance(backs[0], backs[1], xc, xe, target=t.to(DEV))
    finally:
        del model._plain_head
    assert torch.equal(p_c, g_c) and torch.equal(p_e, g_e)              # (the heads do not enter d y / d a)


# ------------------------------------------------------------------------------------------------ 3. the chain kernel alone
def _bimodal(A_c, A_e, abar):
    from mfvit import _lib
    h = _lib.lib()
    mc = torch.stack(A_c).float().to(DEV).contiguous()
    me = torch.stack(A_e).float().to(DEV).contiguous()
    ab = abar.float().to(DEV).contiguous()
    Lc, B, T, _ = mc.shape
    out = torch.empty(4, B, T - 1, device=DEV)
    scratch = torch.empty(h.mfvit_bimodal_relevance_scratch_bytes(B, T), device=DEV, dtype=torch.uint8)
    rc = h.mfvit_bimodal_relevance(B, T, Lc, me.shape[0], mc.data_ptr(), me.data_ptr(), ab.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    # the reference sees exactly the f32 inputs the kernel saw
    return out, [a.double().cpu() for a in mc], [a.double().cpu() for a in me], ab.double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Lc,Le,zero_c,zero_e", [(197, 2, 3, 2, 50, 130), (33, 3, 2, 3, 32, 0), (5, 2, 2, 2, 0, 3), (1100, 1, 1, 2, 1099, 600)])
def test_bimodal_relevance_kernel_matches_float64_on_synthetic_maps(T, B, Lc, Le, zero_c, zero_e):
    # zero_c / zero_e: a token whose map rows are all zero (n = 0: its Rbar row is e_j; token 0: Rbar[0,0] = 1)
    A_c = R.synthetic_maps(500 + T, Lc, B, T, scale=4.0 / T, zero_token=zero_c)
    A_e = R.synthetic_maps(600 + T, Le, B, T, scale=4.0 / T, zero_token=zero_e)
    g = torch.Generator().manual_seed(700 + T)
    abar = torch.rand(2, B, T, generator=g, dtype=torch.float64) * 0.1
    out, A_c, A_e, abar = _bimodal(A_c, A_e, abar)
    want = R.explicit_cross_relevance(A_c, A_e, abar[0], abar[1])
    errs = [R.rel_err(out[k], want[k]) for k in range(4) if float(want[k].abs().max()) > 0]
    zeros = [k for k in range(4) if float(want[k].abs().max()) == 0]                     # (a zero cls row: r[1:] = 0 exactly)
    assert all(float(out[k].abs().max()) == 0 for k in zeros) and len(errs) >= 3
    print(f"[bimodal chain T={T}] cc / ce / ec / ee {', '.join(f'{e:.1e}' for e in errs)}")
    assert max(errs) < GATE["chain"], errs
    out2, *_ = _bimodal(A_c, A_e, abar)
    assert torch.equal(out, out2)


# ------------------------------------------------------------------------------------------------ 4. end to end against the float64 model
def _ref_cross(vit_p, fus_p, imgs, H, t):
    fp = _d(fus_p, True)
    vp = [_d(p, True) for p in vit_p]
    fc, pc = R.ref_features(vp[0], imgs[0].double(), ENC_HEADS)
    fe, pe = R.ref_features(vp[1], imgs[1].double(), ENC_HEADS)
    fused, kept = R.fus_forward_probs(fp, fc, fe, H)
    out = fused + ref_vit.head_linear(vp[0], fc[:, 0]) + ref_vit.head_linear(vp[1], fe[:, 0])
    out.gather(1, t.view(-1, 1)).sum().backward()
    return R.explicit_cross_relevance(R.encoder_maps(pc), R.encoder_maps(pe), R.abar_of(kept[0][0]), R.abar_of(kept[0][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_cross_relevance_matches_the_float64_model(case):
    model, backs, vit_p, fus_p, imgs, t = _ca(case)
    assert backs[0].precision == "bf16x3"
    B, (h, w) = CASES[case]["B"], CASES[case]["img"]
    want = _ref_cross(vit_p, fus_p, imgs, CASES[case]["heads"], t)
    got = model.cross_relevance(backs[0], backs[1], imgs[0].to(DEV), imgs[1].to(DEV), target=t.to(DEV))
    assert len(got) == 4 and all(g.shape == (B, h // 16, w // 16) and g.dtype == torch.float32 and not g.requires_grad for g in got)
    errs = [R.rel_err(g.reshape(B, -1), r) for g, r in zip(got, want)]
    print(f"[cross relevance {case}] cc / ce / ec / ee {', '.join(f'{e:.1e}' for e in errs)}")
    assert max(errs) < GATE["cross"], errs


# ------------------------------------------------------------------------------------------------ 5. the same bits on a repeated call
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a", "b"])
def test_same_bits_on_a_repeated_call(case):
    model, backs, _, _, imgs, t = _ca(case)
    xc, xe, tt = imgs[0].to(DEV), imgs[1].to(DEV), t.to(DEV)
    for call in (lambda: model.get_exchange_attention(backs[0], backs[1], xc, xe)[0],
                 lambda: model.get_exchange_attention(backs[0], backs[1], xc, xe, head_fusion="mean")[0],
                 lambda: model.exchange_relevance(backs[0], backs[1], xc, xe, target=tt),
                 lambda: model.cross_relevance(backs[0], backs[1], xc, xe, target=tt)):
        one, two = call(), call()
        assert all(torch.equal(a, b) for a, b in zip(one, two))
        assert all(bool(torch.isfinite(a).all()) for a in one)


# ------------------------------------------------------------------------------------------------ 6. no side effects
@pytest.mark.gpu
def test_forward_relevance_and_a_training_step_after_the_new_calls_are_bit_identical_to_a_fresh_models():
    y = torch.tensor([0, 1], device=DEV)
    runs = []
    for call in (True, False):
        model, backs, _, _, imgs, t = _ca("a", fresh=True)
        xc, xe, tt = imgs[0].to(DEV), imgs[1].to(DEV), t.to(DEV)
        model.train()
        for b in backs:
            b.train()
        if call:
            cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
            caches = [b._feat_cache for b in backs]
            model.get_exchange_attention(backs[0], backs[1], xc, xe, head_fusion="max")
            model.exchange_relevance(backs[0], backs[1], xc, xe)
            model.cross_relevance(backs[0], backs[1], xc, xe, target=tt)
            torch.cuda.synchronize()
            assert all(p.grad is None for m in (model, *backs) for p in m.parameters())
            assert all(getattr(b, "_grad_arena", None) is None for b in backs)
            assert model.training and all(b.training for b in backs)
            assert all(b._feat_cache is c for b, c in zip(backs, caches))
            assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
        with torch.no_grad():
            fwd = [o.clone() for o in model(backs[0], backs[1], xc, xe)]
        rel = model.attention_relevance(backs[0], backs[1], xc, xe, target=tt)
        fused, x_c, x_e = model(backs[0], backs[1], xc, xe)
        F.cross_entropy(fused + x_c + x_e, y).backward()
        torch.cuda.synchronize()
        grads = [p.grad.clone() for m in (model, *backs) for p in m.parameters() if p.requires_grad]
        runs.append((fwd, rel, fused.detach().clone(), grads))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert torch.equal(runs[0][2], runs[1][2])
    assert len(runs[0][3]) == len(runs[1][3]) > 50
    assert all(torch.equal(a, b) for a, b in zip(runs[0][3], runs[1][3]))
