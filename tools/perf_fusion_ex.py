#!/usr/bin/env python3
"""Fusion-only forward / backward times of Fus_CrossViT at B = 128, T = 197 (features given, backbone heads fused, d features computed):
the default shape (dim 384, 3 heads, one layer, cls) and the _ex configurations.  Median of --iters timed iterations after --warmup, HIP
events around each phase.  One JSON line per configuration.
    python tools/perf_fusion_ex.py [--iters 50] [--warmup 10] [--configs default,d768,L2,mean]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
FUS_MOD = ("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
           "changemodelinputlocation_std002_sum")
CONFIGS = {"default": dict(), "d768": dict(dim=768), "d768_h12": dict(dim=768, heads=12), "L2": dict(depth=2), "mean": dict(pool="mean"),
           "d768_L2_mean": dict(dim=768, depth=2, pool="mean")}


class Provider(torch.nn.Module):
    def __init__(self, feats, C):
        super().__init__()
        self.feats = feats
        self.head = torch.nn.Linear(feats.shape[-1], C)

    def features3D(self, img):
        return self.feats

    def forward(self, img):
        return self.head(self.feats[:, 0])


def time_config(name, dim=384, heads=3, depth=1, pool="cls", B=128, T=197, iters=50, warmup=10):
    fus = importlib.import_module(FUS_MOD)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    fc = torch.randn(B, T, dim, generator=g).to(dev).requires_grad_(True)
    fe = torch.randn(B, T, dim, generator=g).to(dev).requires_grad_(True)
    vc, ve = Provider(fc, 3).to(dev), Provider(fe, 3).to(dev)
    vc.feats, ve.feats = fc, fe
    model = fus.Fus_CrossViT(vc, ve, small_dim=dim, large_dim=dim, heads=heads, cross_attn_depth=depth, pool=pool).to(dev)
    r = torch.randn(B, 3, device=dev)
    fwd, bwd = [], []
    for it in range(warmup + iters):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        fused, xc, xe = model(vc, ve, None, None)
        e1.record()
        ((fused + xc + xe) * r).sum().backward()
        e2.record()
        torch.cuda.synchronize()
        if it >= warmup:
            fwd.append(e0.elapsed_time(e1) * 1e3)
            bwd.append(e1.elapsed_time(e2) * 1e3)
        for p in list(model.parameters()) + [fc, fe, vc.head.weight, vc.head.bias, ve.head.weight, ve.head.bias]:
            p.grad = None
    med = lambda v: sorted(v)[len(v) // 2]
    return dict(config=name, dim=dim, heads=heads, depth=depth, pool=pool, B=B, T=T, fwd_us=round(med(fwd), 1), bwd_us=round(med(bwd), 1),
                total_us=round(med(fwd) + med(bwd), 1))


def time_ca_vit_base(B, iters, warmup, heads=3, depth=1, pool="cls"):
    import vits
    fus = importlib.import_module(FUS_MOD)
    dev = torch.device("cuda:0")
    backs = [vits.vit_base(num_classes=3).to(dev) for _ in range(2)]
    model = fus.Fus_CrossViT(backs[0], backs[1], small_dim=768, large_dim=768, heads=heads, cross_attn_depth=depth, pool=pool).to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    img_c, img_e = torch.randn(B, 3, 224, 224, generator=g).to(dev), torch.randn(B, 3, 224, 224, generator=g).to(dev)
    target = torch.randint(0, 3, (B,), generator=g).to(dev)
    params = [p for m in (backs[0], backs[1], model) for p in m.parameters()]
    ms = []
    for it in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fused, xc, xe = model(backs[0], backs[1], img_c, img_e)
        torch.nn.functional.cross_entropy(fused + xc + xe, target).backward()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
        for p in params:
            p.grad = None
    med = sorted(ms)[len(ms) // 2]
    return dict(workload="ca_vit_base", B=B, heads=heads, depth=depth, pool=pool, step_ms=round(med, 3), pairs_per_s=round(B / med * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--configs", default="default,d768,d768_h12,L2,mean,d768_L2_mean")
    ap.add_argument("--ca-vit-base", type=int, default=0)
    a = ap.parse_args()
    if a.ca_vit_base:
        print(json.dumps(time_ca_vit_base(a.ca_vit_base, a.iters, a.warmup)), flush=True)
        return
    for name in a.configs.split(","):
        print(json.dumps(time_config(name, iters=a.iters, warmup=a.warmup, **CONFIGS[name])), flush=True)


if __name__ == "__main__":
    main()
