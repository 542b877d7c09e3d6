"""Cost of the class-specific attention relevance (include/mfvit.h, mfvit_vit_backward_rel; csrc/attention_maps.hip) on vit_small (development
aid, not the contract bench).

Configurations, each one call = what it names, timed with device events after a warm-up, in interleaved rounds on one GPU (A B C ... A B C ...)
so that a drift of the clock hits all of them alike; the median of the rounds is reported, and each call as a ratio to saliency_frozen:
    fwd                  a plain no-grad forward (model(x))
    saliency_frozen      forward + CE + backward of a frozen backbone with img.requires_grad (the image gradient, data-gradient chain only)
    attention_relevance  attention_relevance(x): forward with saved activations, the head's gradient, the data-gradient chain with a relevance
                         step behind every block's attention backward   (estimate: about 1.5 x saliency_frozen)
    ca_relevance         Fus_CrossViT.attention_relevance over two vit_small encoders (cls pool, one exchange layer)

    python tools/perf_relevance.py [--batch 128] [--precision bf16x3] [--steps 20] [--warmup 5] [--rounds 5]
                                   [--out profiles/relevance_perf.json]
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
import torch.nn.functional as F  # noqa: E402
import vits  # noqa: E402

FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
ESTIMATE = {"attention_relevance": 1.5}          # ratio to saliency_frozen


def freeze_all_but_head(m):
    for name, p in m.named_parameters():
        if name not in ("head.weight", "head.bias"):
            p.requires_grad = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relevance_perf.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.randn(a.batch, 3, 224, 224, device=dev)
    xe = torch.randn(a.batch, 3, 224, 224, device=dev)
    y = (torch.arange(a.batch) % 3).to(dev)
    m = vits.vit_small(num_classes=3, precision=a.precision).to(dev).eval()
    frozen = vits.vit_small(num_classes=3, precision=a.precision).to(dev).eval()
    freeze_all_but_head(frozen)
    backs = [vits.vit_small(num_classes=3, precision=a.precision).to(dev).eval() for _ in range(2)]
    fus = importlib.import_module(FUS_MOD).Fus_CrossViT(backs[0], backs[1]).to(dev).eval()

    def fwd():
        with torch.no_grad():
            m(x)

    def saliency():
        xi = x.detach().requires_grad_(True)
        F.cross_entropy(frozen(xi), y).backward()

    configs = {"fwd": fwd, "saliency_frozen": saliency, "attention_relevance": lambda: m.attention_relevance(x),
               "ca_relevance": lambda: fus.attention_relevance(backs[0], backs[1], x, xe)}
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
    ratio = {k: round(med[k] / med["saliency_frozen"], 4) for k in configs if k != "saliency_frozen"}
    res = {
        "what": "vit_small class-specific relevance cost: median ms per call over interleaved rounds (device events), ratio to the frozen-backbone "
                "image-gradient step",
        "device": torch.cuda.get_device_name(0),
        "batch": a.batch, "precision": a.precision, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
        "ratio_to_saliency_frozen": ratio,
        "estimate_ratio_to_saliency_frozen": ESTIMATE,
        "within_estimate": {k: ratio[k] <= v for k, v in ESTIMATE.items()},
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
