"""Cost of the image gradient (include/mfvit.h, mfvit_vit_backward_ex) on vit_small (development aid, not the contract bench).

Configurations, each one step = what it names, timed with device events after a warm-up, in interleaved rounds on one GPU (A B C ... A B C ...)
so that a drift of the clock hits all of them alike; the median of the rounds and their spread are reported:
    fwd                  (a) forward only (no autograd graph)
    saliency_frozen      (b) forward + CE + backward with a frozen backbone (the reference's fine-tune freezing), img.requires_grad: the
                             data-gradient-only backward
    train                (c) forward + CE + full backward
    train_img_grad       (c) the same with img.requires_grad (parameter gradients + d loss / d img)
    ca_frozen_img_grad   (d) the two-stream Fus_CrossViT CA step (sum of the three logits -> CE) with frozen backbones, both images requiring
                             gradients

    python tools/perf_input_grad.py [--batch 128] [--precision bf16x3] [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/input_grad_perf.json]
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
import vits  # noqa: E402
from mfvit.losses import cross_entropy  # noqa: E402

FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grad_perf.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.randn(a.batch, 3, 224, 224, device=dev)
    xe = torch.randn(a.batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 3, (a.batch,), device=dev)

    train = vits.vit_small(num_classes=3, precision=a.precision).to(dev)
    frozen = vits.vit_small(num_classes=3, precision=a.precision).to(dev)
    frozen.load_state_dict(train.state_dict())
    freeze_all_but_head(frozen)
    backs = [vits.vit_small(num_classes=3, precision=a.precision).to(dev) for _ in range(2)]
    for b in backs:
        freeze_all_but_head(b)
    ca = importlib.import_module(FUS_MOD).Fus_CrossViT(backs[0], backs[1]).to(dev)

    def fwd():
        with torch.no_grad():
            train(x)

    def step(m, want_img):
        def run():
            m.zero_grad(set_to_none=True)
            xi = x.detach().requires_grad_(want_img)
            loss, _ = cross_entropy(m(xi), y)
            loss.backward()
        return run

    def ca_step():
        ca.zero_grad(set_to_none=True)
        for b in backs:
            b.zero_grad(set_to_none=True)
        xc, xn = x.detach().requires_grad_(True), xe.detach().requires_grad_(True)
        fused, x_c, x_e = ca(backs[0], backs[1], xc, xn)
        loss, _ = cross_entropy(fused + x_c + x_e, y)
        loss.backward()

    configs = {"fwd": fwd, "saliency_frozen": step(frozen, True), "train": step(train, False), "train_img_grad": step(train, True),
               "ca_frozen_img_grad": ca_step}
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
    res = {
        "what": "vit_small image-gradient cost: median ms per step over interleaved rounds (device events)",
        "device": torch.cuda.get_device_name(0),
        "batch": a.batch, "precision": a.precision, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
        "ratio_b_over_c": round(med["saliency_frozen"] / med["train_img_grad"], 4),
        "overhead_c_img_grad": round(med["train_img_grad"] / med["train"] - 1.0, 4),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
