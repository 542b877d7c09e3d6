"""Cost of training-mode regularisation on the vit_small single-stream train step (development aid, not the contract bench).

Step = forward (features3D -> head), cross-entropy, backward, at B images in one precision.  Configurations: all rates 0 (today's kernels),
drop_path_rate 0.1 alone (the DeiT / MoCo-v3 fine-tune recipe), and every site at once.  The configurations are timed in interleaved rounds
on one GPU (A B C A B C ...), so a drift of the clock hits all of them alike; the median of the rounds and their spread are reported.

    python tools/perf_drop_path.py [--batch 128] [--precision bf16x3] [--steps 20] [--rounds 5] [--out profiles/drop_path_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
import vits  # noqa: E402
from mfvit.losses import cross_entropy  # noqa: E402

CONFIGS = {
    "rates_0": {},
    "drop_path_0.1": dict(drop_path_rate=0.1),
    "all_sites": dict(drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.randn(a.batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 3, (a.batch,), device=dev)
    models = {}
    for name, kw in CONFIGS.items():
        torch.manual_seed(0)
        models[name] = vits.vit_small(num_classes=3, precision=a.precision, **kw).to(dev).train()

    def step(m):
        logits = m(x)
        loss, _ = cross_entropy(logits, y)
        loss.backward()
        m.zero_grad(set_to_none=True)

    for m in models.values():
        for _ in range(a.warmup):
            step(m)
    torch.cuda.synchronize()
    times = {k: [] for k in models}
    for _ in range(a.rounds):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(m)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    base = statistics.median(times["rates_0"])
    res = {"batch": a.batch, "precision": a.precision, "steps_per_round": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, t in times.items():
        med = statistics.median(t)
        res["configs"][name] = {"rates": CONFIGS[name], "ms_per_step_median": round(med, 3), "ms_per_step_rounds": [round(v, 3) for v in t],
                                "spread_pct": round(100 * (max(t) - min(t)) / med, 2), "ratio_to_rates_0": round(med / base, 4)}
        print(f"{name:>14}: {med:8.3f} ms/step (rounds {min(t):.3f} .. {max(t):.3f}, spread {100 * (max(t) - min(t)) / med:.1f} %)  "
              f"x{med / base:.3f} of rates 0", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
