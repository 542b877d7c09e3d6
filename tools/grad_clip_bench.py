#!/usr/bin/env python3
"""Cost of gradient-norm clipping on the two-encoder CA model of bench.py (mfvit.optim.clip_grad_norm_ against
torch.nn.utils.clip_grad_norm_ on the same gradients, same GPU, same process).

  1. GPU time of each pass (norm passes + finalize, scale passes) between device events, over the optimizer's own chunk tables
  2. host time of a call (the time the call takes to queue its work; the GPU is drained before and after the loop)
  3. the same two figures for torch.nn.utils.clip_grad_norm_ over the same gradient list
  4. the train step at --batches (default 16 and 128 pairs) without clipping, with mfvit's and with torch's, interleaved A / B / C rounds

Both variants clip on every call (max_norm = a quarter of the norm, the gradients are restored between timed loops), and separately with a
bound that never clips.  The gradients are re-read from HBM / Infinity Cache as the loop finds them: what the backward left in a cache
inside a real step shows up only in figure 4.

    python tools/grad_clip_bench.py [--batches 16,128] [--rounds 3] [--steps 30] > profiles/grad_clip_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi-feature-vit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def bench_args(batch):
    import bench
    argv, sys.argv = sys.argv, [argv0, "--batch", str(batch), "--no-cpu-baseline", "--no-extras"]
    try:
        return bench.parse()
    finally:
        sys.argv = argv


argv0 = sys.argv[0]


def gpu_ms(fn, iters, before=None):
    """Median over 5 windows of (device time of `iters` back-to-back calls) / iters."""
    out = []
    for _ in range(5):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def host_us(fn, iters, before=None):
    """Median over 5 windows of the host time of one call (queueing only: nothing in the window waits for the GPU)."""
    out = []
    for _ in range(5):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        out.append(1e6 * (time.perf_counter() - t0) / iters)
        torch.cuda.synchronize()
    return statistics.median(out), min(out), max(out)


def fmt(t, unit):
    return f"{t[0]:9.2f} {unit}  (min {t[1]:.2f}, max {t[2]:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,128")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import bench
    from mfvit import _lib, optim
    from mfvit._lib import check, ptr, stream
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; kernels {_lib.source_hash()[:12]}; medians of 5 windows of {a.iters} calls")
    for bi, batch in enumerate(int(b) for b in a.batches.split(",")):
        run = bench.CaRun(bench_args(batch), dev, 0, "bf16x3", "T")
        opt = run.opt
        for _ in range(5):
            run.step()
        torch.cuda.synchronize()
        params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
        if bi == 0:
            n = sum(p.numel() for p in params)
            saved = [p.grad.clone() for p in params]

            def restore():
                torch._foreach_copy_([p.grad for p in params], saved)
            total = float(optim.grad_norm(opt))
            t_ref = float(torch.nn.utils.clip_grad_norm_(params, 1e30))
            tabs = [opt._table(gi, g)[0] for gi, g in enumerate(opt.param_groups)]
            rows = sum(t.shape[0] for t in tabs)
            print(f"# {len(params)} gradient tensors, {n / 1e6:.2f} M elements, {rows} table rows in {len(tabs)} tables; total norm {total:.6g} (torch: {t_ref:.6g})")
            part = torch.empty(rows, device=dev)
            out = torch.empty(2, device=dev)

            def norm_pass(kind=0):
                r = 0
                for t in tabs:
                    check(lib.mfvit_grad_norm_partials(ptr(t), t.shape[0], kind, part.data_ptr() + 4 * r, stream()), "norm")
                    r += t.shape[0]

            def finalize(max_norm):
                check(lib.mfvit_grad_clip_coef(ptr(part), None, rows, len(params), 0, max_norm, None, ptr(out), stream()), "coef")

            def scale_pass():
                for t in tabs:
                    check(lib.mfvit_grad_scale(ptr(t), t.shape[0], out.data_ptr() + 4, stream()), "scale")
            print("\n## 1. GPU time per pass (device events)")
            t = gpu_ms(norm_pass, a.iters)
            print(f"norm pass, L2 ({len(tabs)} launches, {4 * n / 1e6:.0f} MB read)      {fmt(t, 'ms')}   {4 * n / t[0] / 1e9:.2f} TB/s")
            t = gpu_ms(lambda: norm_pass(1), a.iters)
            print(f"norm pass, inf                                   {fmt(t, 'ms')}   {4 * n / t[0] / 1e9:.2f} TB/s")
            norm_pass()
            t = gpu_ms(lambda: finalize(1e30), a.iters)
            print(f"finalize (1 workgroup, {rows} partials)            {fmt(t, 'ms')}")
            t = gpu_ms(scale_pass, a.iters)
            print(f"scale pass, coefficient 1 (early return)         {fmt(t, 'ms')}")
            finalize(total * 0.999)        # a coefficient just under 1: the gradients shrink by 5 % over 50 calls, the traffic is the real one
            t = gpu_ms(scale_pass, a.iters, before=restore)
            print(f"scale pass, clipping ({8 * n / 1e6:.0f} MB moved)               {fmt(t, 'ms')}   {8 * n / t[0] / 1e9:.2f} TB/s")
            restore()
            print("\n## 2 / 3. whole call: GPU time (device events around the calls) and host time per call")
            k = [0]

            def fresh():
                restore()
                k[0] = 0

            def bound(shrink):          # a bound that drops by 2 % per call stays under the norm the call before left behind: every call clips
                k[0] += 1
                return total * (0.98 ** k[0] if shrink else 4.0)
            for name, shrink in (("never clips (max_norm = 4 x norm)", False), ("clips on every call (max_norm 2 % under the current norm)", True)):
                print(f"-- {name}")
                for who, fn in (("mfvit.optim.clip_grad_norm_     ", lambda: optim.clip_grad_norm_(opt, bound(shrink))),
                                ("torch.nn.utils.clip_grad_norm_  ", lambda: torch.nn.utils.clip_grad_norm_(params, bound(shrink)))):
                    g = gpu_ms(fn, a.iters, before=fresh)
                    h = host_us(fn, a.iters, before=fresh)
                    print(f"{who} GPU {fmt(g, 'ms')}   host {fmt(h, 'us')}")
                restore()
        print(f"\n## 4. train step at {batch} pairs (bf16x3, mode T), {a.rounds} interleaved rounds of {a.steps} steps, ms per step")
        plain = opt.step
        bound = [0.0]

        def ours():
            optim.clip_grad_norm_(opt, bound[0])
            return plain()

        def torchs():
            for gi in range(len(opt.param_groups)):
                opt._pre(gi)
            torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"] if p.grad is not None], bound[0])
            return plain()
        variants = [("no clipping", plain, 0.0), ("mfvit clip, never clips", ours, 1e30), ("mfvit clip, clips every step", ours, 1e-3),
                    ("torch clip, never clips", torchs, 1e30), ("torch clip, clips every step", torchs, 1e-3)]
        times = {v[0]: [] for v in variants}
        for _ in range(a.rounds):
            for name, fn, b in variants:
                opt.step, bound[0] = fn, b
                for _ in range(3):
                    run.step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    run.step()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
        opt.step = plain
        for name, ts in times.items():
            print(f"{name:30s} {statistics.median(ts):8.3f}  (rounds: {', '.join(f'{x:.3f}' for x in ts)})")
        del run, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
