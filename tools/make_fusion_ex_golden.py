#!/usr/bin/env python3
"""Generate tests/golden/fusion_ex_*.npz by running the reference's own Fus_CrossViT / MultiScaleTransformerEncoder (CPU, float64) on
the configurations beyond the defaults: vit_base width (768), heads 6 / 12, cross_attn_depth > 1, multi_scale_enc_depth > 1, pool='mean'.
TEST INFRASTRUCTURE ONLY.  Run from the repo root:   python tools/make_fusion_ex_golden.py
Reuses oracle/make_golden.py (imported, not modified): its reference path setup, timm stub, seeded tensors and sampling helpers.
Stored: seeds and shapes of the inputs, outputs, sampled gradients (N_PARAM points per parameter gradient, N_ROWS per token tensor; the
sum and absolute sum of every whole tensor as well), and the reference's state_dict key lists.  Data only; every file stays a few 100 kB.

Parameters: state-dict tensor i of a case gets rng_tensor(seed_params * 1000 + i, shape, s) with s = 0.05 for matrices, 0.1 for biases,
and 1 + 0.1 N(0, 1) for LayerNorm weights (tests/test_fusion_ex_gpu.py restates this rule).  Loss: sum(out_k * r_k) over the outputs with
seeded r_k, so every gradient is pinned."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402  (puts the reference on sys.path)

OUT = os.path.join(ROOT, "tests", "golden")
N_PARAM, N_ROWS = 256, 2048

# (name, dim, heads, cross_attn_depth, pool, multi_scale_enc_depth, B, T)
FUS_CASES = [
    ("d384_h3_L2_cls_M1", 384, 3, 2, "cls", 1, 2, 197),
    ("d384_h3_L1_mean_M1", 384, 3, 1, "mean", 1, 2, 197),
    ("d768_h3_L1_cls_M1", 768, 3, 1, "cls", 1, 2, 197),
    ("d768_h12_L2_mean_M2", 768, 12, 2, "mean", 2, 2, 197),
    ("d384_h6_L3_cls_M1", 384, 6, 3, "cls", 1, 2, 197),
    ("d384_h3_L2_cls_M1_T577", 384, 3, 2, "cls", 1, 1, 577),
]
# (name, dim, heads, cross_attn_depth, B, T)
XCH_CASES = [("d768_h3_L1", 768, 3, 1, 2, 197), ("d768_h3_L2", 768, 3, 2, 2, 197)]
# constructor keyword sets whose state_dict key lists are pinned
KEY_CASES = [("dim768", dict(small_dim=768, large_dim=768)), ("L2", dict(cross_attn_depth=2)), ("M2", dict(multi_scale_enc_depth=2)),
             ("mean", dict(pool="mean"))]


def seeded_state(module, seed):
    sd = {}
    for i, (k, v) in enumerate(module.state_dict().items()):
        if v.dim() == 2:
            t = mg.rng_tensor(seed * 1000 + i, tuple(v.shape), 0.05, torch.float64)
        elif k.endswith("bias"):
            t = mg.rng_tensor(seed * 1000 + i, tuple(v.shape), 0.1, torch.float64)
        else:
            t = 1.0 + mg.rng_tensor(seed * 1000 + i, tuple(v.shape), 0.1, torch.float64)
        sd[k] = t
    return sd


class Provider:
    """A 'backbone' returning stored features; its own head is x_S = head(f[:, 0]) (FUS:131,135)."""

    def __init__(self, feats, hw, hb):
        self.feats, self.hw, self.hb = feats, hw, hb

    def features3D(self, img):
        return self.feats

    def __call__(self, img):
        return self.feats[:, 0] @ self.hw.t() + self.hb


def golden_fus(fus, name, D, H, L, pool, M, B, T, seed):
    C = 3
    fc = mg.rng_tensor(seed + 1, (B, T, D), dtype=torch.float64).requires_grad_(True)
    fe = mg.rng_tensor(seed + 2, (B, T, D), dtype=torch.float64).requires_grad_(True)
    hw = [mg.rng_tensor(seed + 3 + i, (C, D), 0.05, torch.float64).requires_grad_(True) for i in range(2)]
    hb = [mg.rng_tensor(seed + 5 + i, (C,), 0.1, torch.float64).requires_grad_(True) for i in range(2)]
    pc, pe = Provider(fc, hw[0], hb[0]), Provider(fe, hw[1], hb[1])
    model = fus.Fus_CrossViT(pc, pe, num_classes=C, small_dim=D, large_dim=D, cross_attn_depth=L, multi_scale_enc_depth=M, heads=H,
                             pool=pool).double()
    model.load_state_dict(seeded_state(model, seed), strict=True)
    fused, x_c, x_e = model(pc, pe, None, None)
    r = [mg.rng_tensor(seed + 7 + i, (B, C), dtype=torch.float64) for i in range(3)]
    loss = (fused * r[0]).sum() + (x_c * r[1]).sum() + (x_e * r[2]).sum()
    loss.backward()
    d = dict(dim=D, heads=H, depth=L, pool=pool, msd=M, B=B, T=T, C=C, seed=seed)
    mg.put(d, "fused", fused, full=True)
    mg.put(d, "x_cxr", x_c, full=True)
    mg.put(d, "x_enh", x_e, full=True)
    mg.put(d, "loss", loss, full=True)
    mg.put(d, "d.f_cxr", fc.grad, n=N_ROWS)
    mg.put(d, "d.f_enh", fe.grad, n=N_ROWS)
    for i, k in enumerate(("hw_cxr", "hw_enh")):
        mg.put(d, "d." + k, hw[i].grad, full=True)
    for i, k in enumerate(("hb_cxr", "hb_enh")):
        mg.put(d, "d." + k, hb[i].grad, full=True)
    for n, p in model.named_parameters():
        if p.grad is None:
            d["nograd." + n] = np.int64(1)     # the dead encoders (FUS:137-139)
        else:
            mg.put(d, "d." + n, p.grad, n=N_PARAM)
    d["keys"] = np.array(list(model.state_dict().keys()))
    np.savez_compressed(os.path.join(OUT, f"fusion_ex_{name}.npz"), **d)
    print(f"fusion_ex_{name}.npz  loss {loss.item():.6f}")


def golden_exchange(fus, name, D, H, L, B, T, seed):
    enc = fus.MultiScaleTransformerEncoder(small_dim=D, large_dim=D, cross_attn_depth=L, cross_attn_heads=H).double()
    enc.load_state_dict(seeded_state(enc, seed), strict=True)
    xs = mg.rng_tensor(seed + 1, (B, T, D), dtype=torch.float64).requires_grad_(True)
    xl = mg.rng_tensor(seed + 2, (B, T, D), dtype=torch.float64).requires_grad_(True)
    xs_o, xl_o = enc(xs, xl)
    r = [mg.rng_tensor(seed + 3 + i, (B, T, D), dtype=torch.float64) for i in range(2)]
    loss = (xs_o * r[0]).sum() + (xl_o * r[1]).sum()
    loss.backward()
    d = dict(dim=D, heads=H, depth=L, B=B, T=T, seed=seed)
    mg.put(d, "xs_out", xs_o, n=N_ROWS)
    mg.put(d, "xl_out", xl_o, n=N_ROWS)
    mg.put(d, "d.xs", xs.grad, n=N_ROWS)
    mg.put(d, "d.xl", xl.grad, n=N_ROWS)
    for n, p in enc.named_parameters():
        mg.put(d, "d." + n, p.grad, n=N_PARAM)
    d["keys"] = np.array(list(enc.state_dict().keys()))
    np.savez_compressed(os.path.join(OUT, f"fusion_ex_xch_{name}.npz"), **d)
    print(f"fusion_ex_xch_{name}.npz  loss {loss.item():.6f}")


def golden_keys(fus):
    d = {}
    dummy = Provider(None, None, None)
    for name, kw in KEY_CASES:
        d[name] = np.array(sorted(fus.Fus_CrossViT(dummy, dummy, **kw).state_dict().keys()))
    np.savez_compressed(os.path.join(OUT, "fusion_ex_keys.npz"), **d)
    print("fusion_ex_keys.npz")


def main():
    import importlib
    mg.install_timm_stub()
    fus = importlib.import_module(mg.FUS_MOD)
    torch.manual_seed(0)
    golden_keys(fus)
    for i, (name, D, H, L, B, T) in enumerate(XCH_CASES):
        golden_exchange(fus, name, D, H, L, B, T, 900 + 10 * i)
    for i, c in enumerate(FUS_CASES):
        golden_fus(fus, *c, seed=700 + 10 * i)


if __name__ == "__main__":
    main()
