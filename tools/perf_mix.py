"""Time of the two-stream batch mix (mfvit_batch_mix: Mixup or CutMix of the CXR batch and its enhanced twin in one launch) against the
torch-eager formulation of the same mix (development aid, not the contract bench).

Both are timed in interleaved rounds on one GPU with device events (hip eager hip eager ...); the median of the rounds and their spread are
reported, with the bytes the mix has to move (Mixup: read x_i, read x_j, write = 3 floats per element and stream; CutMix: every element is read
once and written once = 2) and the rate they give.  `--impl hip --rounds 1` under `rocprofv3 --kernel-trace --stats` gives the kernel time alone.

    python tools/perf_mix.py [--batch 128] [--size 224] [--mode mixup|cutmix] [--impl both|hip|eager] [--calls 50] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
from mfvit import ops  # noqa: E402
from mfvit.mixup import Mixup, check_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--mode", choices=("mixup", "cutmix"), default="mixup")
    ap.add_argument("--impl", choices=("both", "hip", "eager"), default="both")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, S = a.batch, a.size
    g = torch.Generator().manual_seed(0)
    x, xe = torch.randn(n, 3, S, S, generator=g).to(dev), torch.randn(n, 3, S, S, generator=g).to(dev)
    mix = Mixup(mixup_alpha=0.8 if a.mode == "mixup" else 0.0, cutmix_alpha=1.0 if a.mode == "cutmix" else 0.0, mode="batch")
    desc, lam = mix.sample_params(n, S, S, g)
    if a.mode == "cutmix":                 # a box of a quarter of the image, wherever the draw put it: the time does not hang on one seed's box
        desc[:, 2:6] = torch.tensor([S // 4 + 1, S // 4 + 1 + S // 2, S // 4 + 3, S // 4 + 3 + S // 2], dtype=torch.int32)
        lam[:] = 0.75
    check_params(desc, lam, n, S, S)
    d_dev, l_dev = desc.to(dev), lam.to(dev)
    partner = desc[:, 0].long().to(dev)
    lam4 = l_dev.view(n, 1, 1, 1)
    yl, yh, xl, xh = desc[0, 2:6].tolist()

    def hip():
        return ops.batch_mix(x, d_dev, l_dev, xe)

    def eager():
        outs = []
        for t in (x, xe):
            if a.mode == "mixup":
                outs.append(lam4 * t + (1.0 - lam4) * t[partner])
            else:
                o = t.clone()
                o[:, :, yl:yh, xl:xh] = t[partner][:, :, yl:yh, xl:xh]
                outs.append(o)
        return outs

    impls = {k: f for k, f in (("hip", hip), ("eager", eager)) if a.impl in ("both", k)}
    if len(impls) == 2:
        for u, v in zip(hip(), eager()):
            err = float((u - v).abs().max())
            assert err <= (4e-6 if a.mode == "mixup" else 0.0), err
    for f in impls.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(a.rounds):
        for k, f in impls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    moved = 2 * (3 if a.mode == "mixup" else 2) * x.numel() * 4
    res = {"what": "two-stream batch mix", "mode": a.mode, "batch": n, "shape": [3, S, S], "bytes_moved": moved,
           "bytes_3_per_element": 2 * 3 * x.numel() * 4, "calls_per_round": a.calls, "rounds": a.rounds}
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = {"us_per_call_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2), "GBps": round(moved / med / 1e3, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
