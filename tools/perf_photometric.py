"""Cost of the photometric chains (aug1 / aug2) of the GPU input pipeline: 2 x 128 views at 224^2 through two_views, against the plain
mocov3 launch (the geometric chain alone) with the same RandomResizedCrop boxes and flips.

    python tools/perf_photometric.py [--out profiles/photometric_perf.txt] [--step-ms MS]

Device time: events around REPS windows of ITERS calls on resident inputs, the two chains alternating; host time: a host clock around
whole two_views calls (descriptor building, uploads, launches) ending in a synchronise.  --step-ms: the MoCo step time of
`bench.py --workload moco` on the same machine, to put the added time against."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import numpy as np
import torch
from mfvit import input_pipeline as ip
from mfvit._lib import check, lib, ptr, stream

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--step-ms", type=float)
ap.add_argument("--pairs", type=int, default=128)
ap.add_argument("--size", type=int, default=224)
args = ap.parse_args()
B, H, W, S = args.pairs, 320, 390, args.size
REPS, ITERS, HBM = 7, 20, 8.0e12
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


rng = np.random.Generator(np.random.PCG64(0))
imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
photo_tf = ip.GpuTransform("imagenet", img_size=S, mocov3=True, photometric=(ip.AUG1, ip.AUG2))
plain_tf = ip.GpuTransform("imagenet", img_size=S, rotate=0, mocov3=True)
pairs = photo_tf.sample_view_pairs(B, torch.Generator().manual_seed(0), [(H, W)] * B)
plain_pairs = [(q[:5], k[:5]) for q, k in pairs]


def spread(v):
    return f"median {statistics.median(v):.1f}, min {min(v):.1f}, max {max(v):.1f}"


# ---- whole calls from the host's side
for tf, pr in ((plain_tf, plain_pairs), (photo_tf, pairs)):      # warm-up: code objects, axis tables, allocator
    for _ in range(2):
        tf.two_views(imgs, pr)
torch.cuda.synchronize()
host = {"plain": [], "photometric": []}
for _ in range(REPS):
    for name, tf, pr in (("plain", plain_tf, plain_pairs), ("photometric", photo_tf, pairs)):
        t0 = time.perf_counter()
        tf.two_views(imgs, pr)
        torch.cuda.synchronize()
        host[name].append(1e3 * (time.perf_counter() - t0))
say(f"two_views, {B} pairs at {S}^2 from {H}x{W} sources, whole call incl. descriptors and the upload of {B * H * W * 3 / 1e6:.1f} MB (ms):")
for name in host:
    say(f"  {name:12s} {spread(host[name])}")
t0 = time.perf_counter()
for _ in range(REPS):
    pd = [ip.photo_descriptor(v[5]) for p in pairs for v in p]
say(f"  photometric descriptors alone (host): {1e3 * (time.perf_counter() - t0) / REPS:.2f} ms for {2 * B} views")

# ---- device time on resident inputs
n = 2 * B
views = [(s, p[0]) for s, p in enumerate(pairs)] + [(s, p[1]) for s, p in enumerate(pairs)]
desc = np.zeros((n, 20), dtype=np.int64)
pdesc = np.zeros((n, 16), dtype=np.int32)
tabs, tab_off, pos = [], {}, 0
for s, (src_i, (flip, _, _, _, (bi, bj, h, w), photo)) in enumerate(views):
    for key in ((w, S), (h, S)):
        if key not in tab_off:
            ks, t = ip.axis_table(*key)
            tab_off[key] = (pos, ks)
            tabs.append(t.reshape(-1))
            pos += t.size
    tx, ty = tab_off[(w, S)], tab_off[(h, S)]
    desc[s] = [src_i * H * W * 3 + (bi * W + bj) * 3, h, w, tx[0], ty[0], tx[1], ty[1], int(flip), 0, 0, 0, 0, 0, 0, 0, 0, W * 3, 0, 0, 0]
    pdesc[s], _ = ip.photo_descriptor(photo)
dev = torch.device("cuda:0")
src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
dsc, pds, tab = (torch.from_numpy(a).to(dev) for a in (desc, pdesc, np.concatenate(tabs)))
out = torch.empty(n, 3, S, S, device=dev)
ws = torch.empty(lib().mfvit_input_photometric_workspace_bytes(n, S), device=dev, dtype=torch.uint8)
mean, std = (ctypes.c_float * 3)(*photo_tf.mean), (ctypes.c_float * 3)(*photo_tf.std)
mp, sp = ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(std, ctypes.c_void_p)


def run_plain():
    check(lib().mfvit_input_transform_rect(ptr(src), ptr(dsc), ptr(tab), n, S, S, S, mp, sp, ptr(out), stream()), "plain")


def run_photo():
    check(lib().mfvit_input_photometric(ptr(src), ptr(dsc), ptr(tab), ptr(pds), n, S, 1, ptr(ws), mp, sp, ptr(out), stream()), "photometric")


for fn in (run_plain, run_photo):
    for _ in range(3):
        fn()
torch.cuda.synchronize()
devt = {"plain": [], "photometric": []}
for _ in range(REPS):
    for name, fn in (("plain", run_plain), ("photometric", run_photo)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        devt[name].append(e0.elapsed_time(e1) * 1e3 / ITERS)
say(f"device time per launch sequence on resident inputs, {n} views ({REPS} windows of {ITERS}, alternating; us):")
for name in devt:
    say(f"  {name:12s} {spread(devt[name])}")
bound = n * 3 * S * S * 4 / HBM * 1e6
med = {k: statistics.median(v) for k, v in devt.items()}
say(f"HBM bound of the float32 output ({n * 3 * S * S * 4 / 1e6:.1f} MB at 8 TB/s): {bound:.1f} us -> plain {bound / med['plain']:.3f}, "
    f"photometric {bound / med['photometric']:.3f} of it")
added = med["photometric"] - med["plain"]
say(f"added device time: {added:.1f} us; added host time: {statistics.median(host['photometric']) - statistics.median(host['plain']):.2f} ms")
if args.step_ms:
    say(f"against a MoCo step of {args.step_ms:.2f} ms ({B} pairs): {100 * added / 1e3 / args.step_ms:.2f} % device time")
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
