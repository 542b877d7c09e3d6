#!/usr/bin/env python3
"""Cost of sharpness-aware minimisation on the two-encoder CA model of bench.py (mfvit.optim.SAM against a torch-foreach restatement of
davda54/sam's first_step / second_step on the same parameters and gradients, same GPU, same process).

  1. GPU time of each pass (norm passes + scale, perturb passes, restore passes) between device events, over SAM's own chunk tables
  2. first_step + second_step minus the base optimizer's step: GPU time (device events) and host time (queueing only), for SAM and ASAM
  3. the same for the foreach restatement (its second_step is the restoring copy alone, so nothing is subtracted)
  4. the full SAM train step at --batch pairs (two forwards, two backwards, first_step, second_step) against two plain steps, interleaved rounds

Perturb and restore undo each other, so the timed loops leave the weights where they were.

    python tools/sam_bench.py [--batch 128] [--rounds 3] [--steps 20] > profiles/sam_bench.txt
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi-feature-vit_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from grad_clip_bench import fmt, gpu_ms, host_us  # noqa: E402


def bench_args(batch):
    import bench
    argv, sys.argv = sys.argv, [sys.argv[0], "--batch", str(batch), "--no-cpu-baseline", "--no-extras"]
    try:
        return bench.parse()
    finally:
        sys.argv = argv


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


class ForeachSAM:
    """davda54/sam on torch's foreach ops: the fastest plain-torch form of its per-tensor loops."""

    def __init__(self, params, rho, adaptive):
        self.params, self.rho, self.adaptive = params, rho, adaptive
        self.old = [torch.empty_like(p) for p in params]

    @torch.no_grad()
    def first_step(self):
        ps = [p.detach() for p in self.params]
        gs = [p.grad for p in self.params]
        t = torch._foreach_mul(torch._foreach_abs(ps), gs) if self.adaptive else gs
        norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(t)))
        scale = self.rho / (norm + 1e-12)
        torch._foreach_copy_(self.old, ps)
        e = torch._foreach_mul(torch._foreach_mul(ps, ps), gs) if self.adaptive else gs
        torch._foreach_add_(ps, torch._foreach_mul(e, scale))

    @torch.no_grad()
    def second_step(self):
        torch._foreach_copy_([p.detach() for p in self.params], self.old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import bench
    from mfvit import _lib, optim
    from mfvit._lib import check, ptr, stream
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    print(f"# {torch.cuda.get_device_name(0)} ({os.uname().nodename}); commit {commit()} + working tree; torch {torch.__version__}; "
          f"kernels {_lib.source_hash()[:12]}; medians of 5 windows of {a.iters} calls")
    run = bench.CaRun(bench_args(a.batch), dev, 0, "bf16x3", "T")
    for _ in range(5):
        run.step()
    torch.cuda.synchronize()
    groups = [[p for p in g["params"] if p.grad is not None] for g in run.opt.param_groups]
    params = [p for g in groups for p in g]
    n = sum(p.numel() for p in params)
    sams = {ad: optim.SAM([{"params": g} for g in groups], optim.Adam, rho=0.05, adaptive=ad, lr=1e-4) for ad in (False, True)}
    for s in sams.values():
        s.before_group = run.opt.before_group
        s.first_step()
        s.second_step()                      # (builds the tables and the base state; one Adam step at lr 1e-4)
    torch.cuda.synchronize()
    tabs = [sams[False]._table(gi, g)[0] for gi, g in enumerate(sams[False].param_groups)]
    rows = sum(t.shape[0] for t in tabs)
    print(f"# {len(params)} gradient tensors, {n / 1e6:.2f} M elements, {rows} table rows in {len(tabs)} tables, batch {a.batch}")
    part = torch.empty(rows, device=dev)
    out = torch.empty(2, device=dev)

    def norm_pass(ad):
        r = 0
        for t in tabs:
            check(lib.mfvit_sam_norm_partials(ptr(t), t.shape[0], ad, part.data_ptr() + 4 * r, stream()), "norm")
            r += t.shape[0]
        check(lib.mfvit_sam_scale(ptr(part), rows, None, ptr(out), stream()), "scale")

    def perturb_pass():
        for t in tabs:
            check(lib.mfvit_sam_perturb(ptr(t), t.shape[0], out.data_ptr() + 4, 0.05, stream()), "perturb")

    def restore_pass():
        for t in tabs:
            check(lib.mfvit_sam_restore(ptr(t), t.shape[0], out.data_ptr() + 4, stream()), "restore")

    def both():
        perturb_pass()
        restore_pass()
    print("\n## 1. GPU time per pass (device events)")
    for ad in (0, 1):
        t = gpu_ms(lambda: norm_pass(ad), a.iters)
        b = (8 if ad else 4) * n
        print(f"norm passes + scale, {'adaptive' if ad else 'plain   '} ({len(tabs) + 1} launches, {b / 1e6:.0f} MB read)   {fmt(t, 'ms')}   {b / t[0] / 1e9:.2f} TB/s")
    norm_pass(0)
    t = gpu_ms(both, a.iters)
    print(f"perturb + restore passes ({24 * n / 1e6:.0f} MB moved)                       {fmt(t, 'ms')}   {24 * n / t[0] / 1e9:.2f} TB/s")
    t = gpu_ms(restore_pass, a.iters)
    print(f"restore passes alone ({8 * n / 1e6:.0f} MB moved)                            {fmt(t, 'ms')}   {8 * n / t[0] / 1e9:.2f} TB/s")

    print("\n## 2 / 3. first_step + second_step, GPU time (device events around the calls) and host time per pair of calls")
    for ad, sam in sams.items():
        base = sam.base_optimizer
        lr = [g["lr"] for g in base.param_groups]
        for g in base.param_groups:
            g["lr"] = 0.0                    # the base step runs its full kernel and moves nothing: the loop stays on the same weights

        def pair():
            sam.first_step()
            sam.second_step()
        fe = ForeachSAM(params, 0.05, ad)

        def fe_pair():
            fe.first_step()
            fe.second_step()
        name = "ASAM" if ad else "SAM "
        res = {}
        for who, fn in (("pair", pair), ("base", base.step), ("foreach", fe_pair)):
            res[who] = (gpu_ms(fn, a.iters), host_us(fn, a.iters))
        print(f"-- {name.strip()}")
        print(f"mfvit.optim.SAM first_step + second_step      GPU {fmt(res['pair'][0], 'ms')}   host {fmt(res['pair'][1], 'us')}")
        print(f"  the base Adam step inside it                GPU {fmt(res['base'][0], 'ms')}   host {fmt(res['base'][1], 'us')}")
        print(f"  SAM's own share (pair - base, medians)      GPU {res['pair'][0][0] - res['base'][0][0]:9.2f} ms                           host "
              f"{res['pair'][1][0] - res['base'][1][0]:9.2f} us")
        print(f"torch foreach first_step + restoring copy     GPU {fmt(res['foreach'][0], 'ms')}   host {fmt(res['foreach'][1], 'us')}")
        for g, v in zip(base.param_groups, lr):
            g["lr"] = v
        del fe
    print(f"\n## 4. train step at {a.batch} pairs (bf16x3, mode T), {a.rounds} interleaved rounds of {a.steps} steps, ms per step")
    sam = sams[False]

    def backward():
        fused, x_c, x_e = run.model(run.backs[0], run.backs[1], run.x, run.xe)
        loss, _ = run._ce(fused + x_c + x_e, run.target)
        loss.backward()
        run.sync.reduce_grads(run.small)

    def sam_step():
        sam.zero_grad(set_to_none=True)
        backward()
        sam.first_step(zero_grad=True)
        backward()
        sam.second_step()
    variants = [("plain step", run.step), ("SAM step", sam_step)]
    times = {v[0]: [] for v in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
    for name, ts in times.items():
        print(f"{name:30s} {statistics.median(ts):8.3f}  (rounds: {', '.join(f'{x:.3f}' for x in ts)})")
    p, s = statistics.median(times["plain step"]), statistics.median(times["SAM step"])
    print(f"SAM step - 2 x plain step      {s - 2 * p:8.3f}  ({s / (2 * p):.3f} x two plain steps)")


if __name__ == "__main__":
    main()
