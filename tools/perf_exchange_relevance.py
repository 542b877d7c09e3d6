"""Cost of the Fus_CrossViT exchange maps and the cross-stream relevance (include/mfvit.h: mfvit_fusion_ex_attention,
mfvit_fusion_ex_grad_attention, mfvit_bimodal_relevance) at the CA bench shape (development aid, not the contract bench).

Configurations, each one call = what it names, timed with device events after a warm-up, in interleaved rounds on one GPU (A B C ... A B C ...)
so that a drift of the clock hits all of them alike; the median of the rounds is reported:
    fwd                     one no-grad forward of the two-stream model
    attention_relevance     the existing per-encoder relevance (no exchange term)
    get_exchange_attention  two evaluation forwards + the exchange forward + the map copy
    exchange_relevance      ... + the exchange backward + the gradient-weighted map
    cross_relevance         two relevance passes that write every block's map + the exchange forward / backward + the chain kernel
and two parts of cross_relevance on their own:
    chain_kernel            mfvit_bimodal_relevance on maps of the same shape
    map_writes              one encoder's relevance pass writing every block's map, minus the same pass keeping the cls row only (x 2 encoders)

    python tools/perf_exchange_relevance.py [--batch 128] [--depth 12] [--precision bf16x3] [--steps 10] [--warmup 3] [--rounds 5]
                                            [--out profiles/exchange_relevance_perf.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
import vits_returnftrs as vits  # noqa: E402
from mfvit.fusion import bimodal_relevance  # noqa: E402

FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exchange_relevance_perf.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    B, L = a.batch, a.depth
    xc, xe = torch.randn(B, 3, 224, 224, device=dev), torch.randn(B, 3, 224, 224, device=dev)
    bc, be = (vits.vit_small(num_classes=3, depth=L, precision=a.precision).to(dev).eval() for _ in range(2))
    model = importlib.import_module(FUS_MOD).Fus_CrossViT(bc, be).to(dev).eval()
    T = bc.num_tokens
    t = torch.zeros(B, dtype=torch.int64, device=dev)
    maps = torch.rand(L, B, T, T, device=dev) * (2.0 / T)
    abar = torch.rand(2, B, T, device=dev) * 0.1
    blocks = list(range(L))

    def fwd():
        with torch.no_grad():
            model(bc, be, xc, xe)

    configs = {
        "fwd": fwd,
        "attention_relevance": lambda: model.attention_relevance(bc, be, xc, xe, target=t),
        "get_exchange_attention": lambda: model.get_exchange_attention(bc, be, xc, xe),
        "exchange_relevance": lambda: model.exchange_relevance(bc, be, xc, xe, target=t),
        "cross_relevance": lambda: model.cross_relevance(bc, be, xc, xe, target=t),
        "chain_kernel": lambda: bimodal_relevance(maps, maps, abar),
        "encoder_relevance_all_maps": lambda: bc._relevance(xc, t, blocks, False),
        "encoder_relevance_cls_row": lambda: bc._relevance(xc, t, [], True),
    }
    for fn in configs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in configs}
    for _ in range(a.rounds):
        for k, fn in configs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    writes = 2 * (med["encoder_relevance_all_maps"] - med["encoder_relevance_cls_row"])
    res = {
        "what": "Fus_CrossViT exchange maps and cross-stream relevance: median ms per call over interleaved rounds (device events)",
        "device": torch.cuda.get_device_name(0),
        "batch": B, "depth": L, "tokens": T, "precision": a.precision, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_rounds": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
        "ratio_to_fwd": {k: round(med[k] / med["fwd"], 3) for k in configs if k != "fwd"},
        "stored_maps_bytes": 4 * 2 * L * B * T * T,
        "share_of_cross_relevance": {"chain_kernel": round(med["chain_kernel"] / med["cross_relevance"], 4),
                                     "map_writes (2 x (all maps - cls row only))": round(writes / med["cross_relevance"], 4)},
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
