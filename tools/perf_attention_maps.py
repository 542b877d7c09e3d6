"""Cost of the attention maps (include/mfvit.h, mfvit_vit_forward_attn; csrc/attention_maps.hip) on vit_small (development aid, not the
contract bench).

Configurations, each one call = what it names, timed with device events after a warm-up, in interleaved rounds on one GPU (A B C ... A B C ...)
so that a drift of the clock hits all of them alike; the median of the rounds is reported, and each map call as a ratio to the forward:
    fwd                  a plain no-grad forward (model(x))
    last_selfattention   get_last_selfattention(x): the forward + the per-head probabilities of the last block   (estimate: <= 1.1 x fwd)
    maps_mean_all        get_attention_maps(x, head_fusion='mean'): the forward + a head-mean map of every block
    rollout_mean         attention_rollout(x): the forward + every block's fused map and row sums + the rollout   (estimate: <= 1.3 x fwd)

    python tools/perf_attention_maps.py [--batch 128] [--precision bf16x3] [--steps 20] [--warmup 5] [--rounds 5]
                                        [--out profiles/attention_maps_perf.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
import vits  # noqa: E402

ESTIMATE = {"last_selfattention": 1.1, "rollout_mean": 1.3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps_perf.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.randn(a.batch, 3, 224, 224, device=dev)
    m = vits.vit_small(num_classes=3, precision=a.precision).to(dev).eval()

    def fwd():
        with torch.no_grad():
            m(x)

    configs = {"fwd": fwd, "last_selfattention": lambda: m.get_last_selfattention(x),
               "maps_mean_all": lambda: m.get_attention_maps(x, head_fusion="mean"), "rollout_mean": lambda: m.attention_rollout(x)}
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
    ratio = {k: round(med[k] / med["fwd"], 4) for k in configs if k != "fwd"}
    res = {
        "what": "vit_small attention-map cost: median ms per call over interleaved rounds (device events), ratio to the no-grad forward",
        "device": torch.cuda.get_device_name(0),
        "batch": a.batch, "precision": a.precision, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
        "ratio_to_fwd": ratio,
        "estimate_ratio_to_fwd": ESTIMATE,
        "within_estimate": {k: ratio[k] <= v for k, v in ESTIMATE.items()},
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
