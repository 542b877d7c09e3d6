"""f-2 measurement, aspect-preserving resize: square (Resize((S, S))) vs maintain-ratio (Resize(S)) vs two-view batches of the
fused input kernel, in one process on realistic non-square sources (128 images, short side 900-1100, aspect ratio 0.75-1.33).

Kernel time: the launch GpuTransform makes, replayed on resident data (CUDA events).  End to end: the whole call (host
descriptors, one H2D copy of the sources, launch), median of several.  Bytes: the f32 output plus the source bytes under each
sample's crop window (the source area the crop maps back to, C^2 / (Sh * Sw) of the image), per view.

    python tools/perf_input_ratio.py [--batch 128] [--iters 20]
"""
import argparse, ctypes, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import numpy as np
import torch
from mfvit import input_pipeline as ip

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
B, S, C = args.batch, 256, 224
rng = np.random.Generator(np.random.PCG64(0))
sizes = []
for _ in range(B):
    short, ratio = int(rng.integers(900, 1101)), float(rng.uniform(0.75, 1.33))
    sizes.append((short, max(short, int(short * ratio))) if rng.random() < 0.5 else (max(short, int(short * ratio)), short))
imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
src_bytes = sum(a.size for a in imgs)
print(f"{B} sources, {src_bytes / 1e6:.1f} MB, sizes {min(min(s) for s in sizes)}..{max(max(s) for s in sizes)}")

# capture the launch arguments of one call (tensors kept alive) so the kernel can be replayed alone
_real_ptr, _real_lib = ip.ptr, ip.lib
captured = {}


class _Capture:
    def __getattr__(self, name):
        fn = getattr(_real_lib(), name)

        def call(*a):
            captured["call"] = (fn, a)
            return fn(*a)
        return call


def capture(fn):
    keep = []
    ip.ptr = lambda t: (keep.append(t), _real_ptr(t))[1]
    ip.lib = lambda: _Capture()
    try:
        out = fn()
    finally:
        ip.ptr, ip.lib = _real_ptr, _real_lib
    torch.cuda.synchronize()
    return out, captured.pop("call"), keep


def kernel_us(call):
    fn, a = call
    for _ in range(3):
        fn(*a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.iters


def e2e_ms(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def report(name, n_out, frames, us, ms):
    touched = sum(C * C * h * w * 3 / (fh * fw) for (h, w), (fh, fw) in frames)
    byt = n_out * 3 * C * C * 4 + touched
    print(f"{name:<14} kernel {us:8.1f} us = {n_out / us * 1e6:8.0f} img/s, {us * 1e3 / (n_out * C * C):.3f} ns/out px; "
          f"bytes {byt / 1e6:7.1f} MB (out {n_out * 3 * C * C * 4 / 1e6:.1f} + src {touched / 1e6:.1f}) -> {byt / us / 1e3:6.0f} GB/s; "
          f"end to end {ms:7.2f} ms = {n_out / ms * 1e3:6.0f} img/s")


sq = ip.GpuTransform("CheXpert-v1.0-small", S, C, 10, True)
mr = ip.GpuTransform("CheXpert-v1.0-small", S, C, 10, True, maintain_ratio=True)
p_sq = sq.sample_params(B, torch.Generator().manual_seed(0))
p_mr = mr.sample_params(B, torch.Generator().manual_seed(0), sizes)
p_2v = mr.sample_view_pairs(B, torch.Generator().manual_seed(0), sizes)

out_sq, call_sq, keep_sq = capture(lambda: sq(imgs, p_sq))
out_mr, call_mr, keep_mr = capture(lambda: mr(imgs, p_mr))
(q, k), call_2v, keep_2v = capture(lambda: mr.two_views(imgs, p_2v))
assert torch.equal(q, mr(imgs, [p[0] for p in p_2v])) and torch.equal(k, mr(imgs, [p[1] for p in p_2v]))

f_sq = [((h, w), (S, S)) for h, w in sizes]
f_mr = [((h, w), mr.frame(h, w)) for h, w in sizes]
# interleaved twice so a drift of the clock shows up as a disagreement between the rounds
for rnd in range(2):
    print(f"round {rnd}")
    report("square", B, f_sq, kernel_us(call_sq), e2e_ms(lambda: sq(imgs, p_sq)))
    report("maintain-ratio", B, f_mr, kernel_us(call_mr), e2e_ms(lambda: mr(imgs, p_mr)))
    report("two-view", 2 * B, f_mr * 2, kernel_us(call_2v), e2e_ms(lambda: mr.two_views(imgs, p_2v)))
    ms2 = e2e_ms(lambda: (mr(imgs, [p[0] for p in p_2v]), mr(imgs, [p[1] for p in p_2v])))
    print(f"{'2 x single':<14} end to end {ms2:7.2f} ms = {2 * B / ms2 * 1e3:6.0f} img/s (what two_views replaces)")
