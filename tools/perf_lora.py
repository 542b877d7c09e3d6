"""Train-step time of the three fine-tuning regimes of one vit_small encoder (development aid, not the contract bench).

One step = zero_grad, forward, CE, backward, AdamW on whatever is trainable; timed with device events after a warm-up, in interleaved rounds on
one GPU (A B C D A B C D ...) so that a drift of the clock hits all cases alike; the median of the rounds and their spread are reported:
    frozen_head   every backbone weight frozen, the head trains (no backward through the encoder at all)
    lora_qv       rank-8 adapters on ("q", "v") of all blocks (mfvit.lora), base frozen: mfvit_vit_backward_lora
    lora_all6     rank-8 adapters on all six targets
    full          every backbone weight trains
Expectation from the code, written down before measuring: lora_qv ~ the frozen-backbone saliency step (forward + data-gradient chain,
profiles/input_grad_perf.json: 9.72 ms at B = 128) + 12 fused-qkv weight-gradient launches (~90 us each at B = 128, an estimate from profiles/) + the
shadow rebuild of every step (the merged arena: one 87 MB device copy, one merge launch, four cast / transpose launches) - about 11 ms; lora_all6 adds
the proj (paired with qkv), fc1 and fc2 weight gradients of every block, i.e. every weight-gradient GEMM of the full step, and saves only the column
sums, the embedding stage and the optimizer's pass over 21.7 M weights.

--root DIR imports the package from another checkout (the parent commit, which has no mfvit.lora: only the cases that exist there run), so that the
two unchanged paths can be measured in alternating processes on one box:
    python tools/perf_lora.py [--batch 128] [--steps 20] [--warmup 5] [--rounds 5] [--cases frozen_head,lora_qv,lora_all6,full] [--root DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--precision", default="bf16x3")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cases", default="frozen_head,lora_qv,lora_all6,full")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
import vits  # noqa: E402
from mfvit.losses import cross_entropy  # noqa: E402
from mfvit.optim import AdamW  # noqa: E402


def make(case):
    m = vits.vit_small(num_classes=3, precision=a.precision).to("cuda:0")
    if case == "frozen_head":
        for name, p in m.named_parameters():
            p.requires_grad = name in ("head.weight", "head.bias")
    elif case.startswith("lora"):
        from mfvit import lora
        lora.add_lora(m, rank=8, alpha=16.0, targets=("q", "v") if case == "lora_qv" else lora.TARGETS)
        with torch.no_grad():               # B = 0 would do for the timing; a trained-looking B keeps every product live
            for name, p in m.named_parameters():
                if "lora_B" in name:
                    p.normal_(std=1e-3)
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-5)
    return m, opt


def main():
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.randn(a.batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 3, (a.batch,), device=dev)
    cases = [c for c in a.cases.split(",") if c]
    models = {c: make(c) for c in cases}

    def step(c):
        m, opt = models[c]
        m.zero_grad(set_to_none=True)
        loss, _ = cross_entropy(m(x), y)
        loss.backward()
        opt.step()

    for c in cases:
        for _ in range(a.warmup):
            step(c)
    torch.cuda.synchronize()
    times = {c: [] for c in cases}
    for _ in range(a.rounds):
        for c in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(c)
            e1.record()
            torch.cuda.synchronize()
            times[c].append(e0.elapsed_time(e1) / a.steps)
    res = {"tool": "tools/perf_lora.py", "root": os.path.relpath(ROOT), "batch": a.batch, "precision": a.precision, "steps": a.steps,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "step_ms": {}}
    for c in cases:
        t = times[c]
        res["step_ms"][c] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4),
                             "rounds": [round(v, 4) for v in t]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
