"""GPU parity of Fus_CrossViT beyond the default shape (dim 768, heads 6 / 12, cross_attn_depth > 1, multi_scale_enc_depth > 1,
pool='mean') against the reference's own outputs (tests/golden/fusion_ex_*.npz, tools/make_fusion_ex_golden.py), a vit_base CA step
against a float64 CPU restatement, the default path's bits through the _ex entry points, and run-to-run reproducibility.
Tolerances as tests/test_fusion_gpu.py: scaled error < 1e-3 on outputs, gradients rtol 2e-3 with the abssum-scaled atol."""
import importlib

import pytest
import torch

from conftest import check_sampled, rng_tensor
from oracle import ref_fusion, ref_vit
from oracle.ref_fusion import fus_ex_fused as ref_fus_forward

pytestmark = pytest.mark.gpu
FUS_MOD = ("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
           "changemodelinputlocation_std002_sum")
FUS_CASES = ["d384_h3_L2_cls_M1", "d384_h3_L1_mean_M1", "d768_h3_L1_cls_M1", "d768_h12_L2_mean_M2", "d384_h6_L3_cls_M1",
             "d384_h3_L2_cls_M1_T577"]
DEV = torch.device("cuda:0")


def scale_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def seeded_state(module, seed, dtype=torch.float32):
    """The parameter rule of tools/make_fusion_ex_golden.py::seeded_state."""
    sd = {}
    for i, (k, v) in enumerate(module.state_dict().items()):
        if v.dim() == 2:
            sd[k] = rng_tensor(seed * 1000 + i, tuple(v.shape), 0.05, dtype)
        elif k.endswith("bias"):
            sd[k] = rng_tensor(seed * 1000 + i, tuple(v.shape), 0.1, dtype)
        else:
            sd[k] = (1.0 + rng_tensor(seed * 1000 + i, tuple(v.shape), 0.1, torch.float64)).to(dtype)
    return sd


def check_grad(g, key, t):
    check_sampled(g, key, t, rtol=2e-3, atol=2e-3 * float(g[f"{key}.abssum"]) / t.numel())


class FeatureProvider(torch.nn.Module):
    def __init__(self, feats, hw, hb):
        super().__init__()
        self.feats = feats
        self.head = torch.nn.Linear(hw.shape[1], hw.shape[0])
        with torch.no_grad():
            self.head.weight.copy_(hw)
            self.head.bias.copy_(hb)

    def features3D(self, img):
        return self.feats

    def forward(self, img):
        return self.head(self.feats[:, 0])


@pytest.mark.parametrize("need_df", [True, False])
@pytest.mark.parametrize("case", FUS_CASES)
def test_fus_crossvit_against_reference_golden(golden, case, need_df):
    g = golden(f"fusion_ex_{case}.npz")
    D, H, L, M, B, T, C, seed = (int(g[k]) for k in ("dim", "heads", "depth", "msd", "B", "T", "C", "seed"))
    pool = str(g["pool"])
    fus = importlib.import_module(FUS_MOD)
    fc = rng_tensor(seed + 1, (B, T, D)).to(DEV).requires_grad_(need_df)
    fe = rng_tensor(seed + 2, (B, T, D)).to(DEV).requires_grad_(need_df)
    hw = [rng_tensor(seed + 3 + i, (C, D), 0.05) for i in range(2)]
    hb = [rng_tensor(seed + 5 + i, (C,), 0.1) for i in range(2)]
    vc, ve = FeatureProvider(fc, hw[0], hb[0]).to(DEV), FeatureProvider(fe, hw[1], hb[1]).to(DEV)
    vc.feats, ve.feats = fc, fe
    model = fus.Fus_CrossViT(vc, ve, num_classes=C, small_dim=D, large_dim=D, cross_attn_depth=L, multi_scale_enc_depth=M, heads=H, pool=pool)
    assert list(model.state_dict().keys()) == list(g["keys"])
    model.load_state_dict(seeded_state(model, seed), strict=True)
    model = model.to(DEV)
    fused, xc, xe = model(vc, ve, None, None)
    r = [rng_tensor(seed + 7 + i, (B, C)).to(DEV) for i in range(3)]
    ((fused * r[0]).sum() + (xc * r[1]).sum() + (xe * r[2]).sum()).backward()
    e_f = [scale_err(t, torch.from_numpy(g[k])) for t, k in ((fused, "fused"), (xc, "x_cxr"), (xe, "x_enh"))]
    assert max(e_f) < 1e-3, e_f
    for n, p in model.named_parameters():
        if f"nograd.{n}" in g:
            assert p.grad is None, n              # a dead encoder (FUS:137-139): never in the graph
        else:
            check_grad(g, "d." + n, p.grad)
    for k, t in (("hw_cxr", vc.head.weight), ("hw_enh", ve.head.weight), ("hb_cxr", vc.head.bias), ("hb_enh", ve.head.bias)):
        assert scale_err(t.grad, torch.from_numpy(g["d." + k])) < 1e-3, k
    if need_df:
        check_grad(g, "d.f_cxr", fc.grad)
        check_grad(g, "d.f_enh", fe.grad)
    else:
        assert fc.grad is None and fe.grad is None


def test_dead_encoders_have_no_gradient(golden):
    g = golden("fusion_ex_d768_h12_L2_mean_M2.npz")
    assert any(k.startswith("nograd.multi_scale_transformers.0.") for k in g.files)
    assert not any(k.startswith("nograd.multi_scale_transformers.1.") for k in g.files)
    fus = importlib.import_module(FUS_MOD)
    fc = rng_tensor(5, (2, 197, 768)).to(DEV)
    v = FeatureProvider(fc, torch.zeros(3, 768), torch.zeros(3)).to(DEV)
    v.feats = fc
    model = fus.Fus_CrossViT(v, v, small_dim=768, large_dim=768, heads=12, cross_attn_depth=2, multi_scale_enc_depth=2, pool="mean").to(DEV)
    fused, xc, xe = model(v, v, None, None)
    (fused.sum() + xc.sum()).backward()
    for n, p in model.named_parameters():
        assert (p.grad is None) == n.startswith("multi_scale_transformers.0."), n


@pytest.mark.parametrize("case", ["d768_h3_L1", "d768_h3_L2"])
def test_standalone_exchange_against_reference_golden(golden, case):
    g = golden(f"fusion_ex_xch_{case}.npz")
    D, H, L, B, T, seed = (int(g[k]) for k in ("dim", "heads", "depth", "B", "T", "seed"))
    fus = importlib.import_module(FUS_MOD)
    enc = fus.MultiScaleTransformerEncoder(small_dim=D, large_dim=D, cross_attn_depth=L, cross_attn_heads=H)
    assert list(enc.state_dict().keys()) == list(g["keys"])
    enc.load_state_dict(seeded_state(enc, seed), strict=True)
    enc = enc.to(DEV)
    xs = rng_tensor(seed + 1, (B, T, D)).to(DEV).requires_grad_(True)
    xl = rng_tensor(seed + 2, (B, T, D)).to(DEV).requires_grad_(True)
    xs_o, xl_o = enc(xs, xl)
    r = [rng_tensor(seed + 3 + i, (B, T, D)).to(DEV) for i in range(2)]
    ((xs_o * r[0]).sum() + (xl_o * r[1]).sum()).backward()
    check_sampled(g, "xs_out", xs_o, rtol=1e-3, atol=1e-4)
    check_sampled(g, "xl_out", xl_o, rtol=1e-3, atol=1e-4)
    check_grad(g, "d.xs", xs.grad)
    check_grad(g, "d.xl", xl.grad)
    for n, p in enc.named_parameters():
        check_grad(g, "d." + n, p.grad)


def vit_base_ca(precision, L=1, pool="cls", M=1, heads=3, seed=1801):
    import vits
    fus = importlib.import_module(FUS_MOD)
    bb = []
    for i in range(2):
        m = vits.vit_base(num_classes=3, depth=2, precision=precision)
        m.load_state_dict(ref_vit.seeded_params(seed + i, arch="vit_base", num_classes=3, depth=2), strict=True)
        bb.append(m.to(DEV))
    model = fus.Fus_CrossViT(bb[0], bb[1], small_dim=768, large_dim=768, heads=heads, cross_attn_depth=L, multi_scale_enc_depth=M, pool=pool)
    model.load_state_dict(seeded_state(model, seed + 2), strict=True)
    return bb, model.to(DEV)


def ca_step(bb, model, seed=1811):
    B = 3
    img_c, img_e = rng_tensor(seed, (B, 3, 224, 224)).to(DEV), rng_tensor(seed + 1, (B, 3, 224, 224)).to(DEV)
    target = torch.tensor([2, 0, 1], device=DEV)
    fused, xc, xe = model(bb[0], bb[1], img_c, img_e)
    out = fused + xc + xe
    loss = torch.nn.functional.cross_entropy(out, target)
    loss.backward()
    return img_c, img_e, target, out, loss


@pytest.mark.parametrize("precision,tol_g", [("fp32", 1e-3), ("bf16x3", 2e-3)])
def test_vit_base_ca_step_against_float64_restatement(precision, tol_g):
    bb, model = vit_base_ca(precision)
    img_c, img_e, target, out, loss = ca_step(bb, model)
    pb = [{k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()} for m in bb]
    pf = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    fc, fe = ref_vit.features3d(pb[0], img_c.double().cpu()), ref_vit.features3d(pb[1], img_e.double().cpu())
    out_r = ref_fus_forward(pf, fc, fe, 3, 1, "cls", 1) + ref_vit.head_linear(pb[0], fc[:, 0]) + ref_vit.head_linear(pb[1], fe[:, 0])
    loss_r = torch.nn.functional.cross_entropy(out_r, target.cpu())
    loss_r.backward()
    assert scale_err(out, out_r) < 1e-3 and abs(loss.item() - loss_r.item()) < 1e-3 * max(1.0, abs(loss_r.item()))
    assert torch.equal(out.argmax(1).cpu(), out_r.argmax(1))
    for m, p in ((bb[0], pb[0]), (bb[1], pb[1]), (model, pf)):
        for n, t in m.named_parameters():
            if not t.requires_grad:
                continue
            e = scale_err(t.grad, p[n].grad)
            assert e < tol_g, (n, e)


def test_ex_entry_points_reproduce_the_default_path_bits():
    from mfvit import _lib
    from mfvit._lib import lib, ptr, stream
    from mfvit.fusion import fusion_cfg
    B, T, D, C = 128, 197, 384, 3
    cfg = fusion_cfg(B, T, C)
    n = lib().mfvit_fusion_param_count(cfg)
    assert lib().mfvit_fusion_ex_param_count(cfg, 1, 0) == n
    params = ref_fusion.seeded_fusion_params(1901)
    flat = torch.cat([v.flatten() for v in params.values()]).to(DEV)
    assert flat.numel() == n
    fc, fe = rng_tensor(1902, (B, T, D)).to(DEV), rng_tensor(1903, (B, T, D)).to(DEV)
    hw = [rng_tensor(1904 + i, (C, D), 0.05).to(DEV) for i in range(2)]
    hb = [rng_tensor(1906 + i, (C,), 0.1).to(DEV) for i in range(2)]
    dfu, dxc, dxe = (rng_tensor(1908 + i, (B, C)).to(DEV) for i in range(3))

    def run(ex):
        ws = torch.empty(lib().mfvit_fusion_workspace_bytes(cfg), device=DEV, dtype=torch.uint8)
        fused, xc, xe = (torch.empty(B, C, device=DEV) for _ in range(3))
        gp, dhw_c, dhb_c, dhw_e, dhb_e = torch.zeros_like(flat), torch.zeros(C, D, device=DEV), torch.zeros(C, device=DEV), \
            torch.zeros(C, D, device=DEV), torch.zeros(C, device=DEV)
        dfc, dfe = torch.empty_like(fc), torch.empty_like(fe)
        fa = (ptr(flat), ptr(fc), ptr(fe), ptr(hw[0]), ptr(hb[0]), ptr(hw[1]), ptr(hb[1]), ptr(ws), ptr(fused), ptr(xc), ptr(xe), stream())
        ba = (ptr(flat), ptr(fc), ptr(fe), ptr(hw[0]), ptr(hw[1]), ptr(ws), ptr(dfu), ptr(dxc), ptr(dxe), ptr(gp), ptr(dfc), ptr(dfe),
              ptr(dhw_c), ptr(dhb_c), ptr(dhw_e), ptr(dhb_e), stream())
        if ex:
            _lib.check(lib().mfvit_fusion_ex_forward(cfg, 1, 0, *fa), "ex fwd")
            _lib.check(lib().mfvit_fusion_ex_backward(cfg, 1, 0, *ba), "ex bwd")
        else:
            _lib.check(lib().mfvit_fusion_forward(cfg, *fa), "fwd")
            _lib.check(lib().mfvit_fusion_backward(cfg, *ba), "bwd")
        torch.cuda.synchronize()
        return fused, xc, xe, gp, dfc, dfe, dhw_c, dhb_c, dhw_e, dhb_e

    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


def test_vit_base_L2_mean_step_is_bit_reproducible():
    runs = []
    for _ in range(2):
        bb, model = vit_base_ca("bf16x3", L=2, pool="mean", heads=12)
        _, _, _, out, loss = ca_step(bb, model)
        grads = [p.grad.clone() for m in (bb[0], bb[1], model) for p in m.parameters() if p.grad is not None]
        runs.append((out.detach().clone(), loss.detach().clone(), grads))
    (o0, l0, g0), (o1, l1, g1) = runs
    assert torch.equal(o0, o1) and torch.equal(l0, l1) and len(g0) == len(g1) > 0
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
