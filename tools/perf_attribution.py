"""Times of gradient attribution (mfvit.attribution; csrc/attribution.hip) against the torch composition its three kernels replace and against
the model passes it cannot avoid (development aid, not the contract bench).  Three measurements, each in interleaved rounds on one GPU with
device events (ours, theirs, ours, theirs ...), median and spread of the rounds:

  encoder  integrated_gradients of one VisionTransformerMoCo (steps + 1 path points, max_batch = B: one point per forward) against the same
           call with the three attribution launches stubbed out: its steps + 1 saliency steps (evaluation forward, head, data-gradient-only
           backward) alone.
  kernels  what the three kernels do in such a call - per step mfvit_attr_inputs and mfvit_attr_accumulate, at the end mfvit_attr_finish -
           against the torch composition on the same inputs: per step a lerp and an in-place add, then mul, sum(1), avg_pool2d * 256 and a
           double sum.  Results compared before the timing.
  fusion   Fus_CrossViT.integrated_gradients (both streams along the joint path) against its forward and backward passes alone, as above.

    python tools/perf_attribution.py [--batch 64] [--size 224] [--steps 20] [--depth 12] [--calls 2] [--rounds 5] [--out profiles/attribution_bench.txt]
"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from mfvit import attribution  # noqa: E402

FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def rounds(impls, calls, n_rounds, warmup=2):
    """{name: [us per call of every round]}, the implementations alternated inside every round."""
    for f in impls.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in impls}
    for _ in range(n_rounds):
        for k, f in impls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def report(lines, title, times, extra=""):
    lines.append(title)
    for k, t in times.items():
        lines.append(f"  {k:<34s} median {statistics.median(t):10.1f} us   min {min(t):10.1f}   max {max(t):10.1f}   ({len(t)} rounds)")
    if extra:
        lines.append("  " + extra)


class passes_alone:
    """The attribution calls with their three launches stubbed out: preallocated buffers are handed back, nothing is launched."""

    def __init__(self, x):
        B, C, H, W = x.shape
        self.x = x
        self.fin = (torch.zeros(B, H // 16, W // 16, device=x.device), None, torch.zeros(B, device=x.device, dtype=torch.float64))

    def __enter__(self):
        self.saved = (attribution.attr_inputs, attribution.attr_accumulate, attribution.attr_finish)
        attribution.attr_inputs = lambda x, base, alpha, *a: self.x.view(1, *self.x.shape).expand(alpha.shape[0], *self.x.shape)
        attribution.attr_accumulate = lambda *a: None
        attribution.attr_finish = lambda *a: self.fin

    def __exit__(self, *exc):
        attribution.attr_inputs, attribution.attr_accumulate, attribution.attr_finish = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, steps = a.batch, a.size, a.steps
    S = steps + 1
    g = torch.Generator().manual_seed(0)
    x, xe = torch.randn(B, 3, H, H, generator=g).to(dev), torch.randn(B, 3, H, H, generator=g).to(dev)
    base = torch.tensor([0.1, -0.2, 0.3], device=dev)
    lines = [f"gradient attribution: B = {B}, {H} x {H}, steps = {steps} (trapezoid: {S} path points), vit_small depth {a.depth}, bf16x3, "
             f"device {torch.cuda.get_device_name(0)}"]

    # ---------------------------------------------------------------------------------- one encoder
    import vits
    torch.manual_seed(0)
    m = vits.vit_small(num_classes=3, depth=a.depth, img_size=H, precision="bf16x3").to(dev).eval()

    def whole():
        return attribution.integrated_gradients(m, x, 1, base, steps=steps, max_batch=B)

    def alone():
        with passes_alone(x):
            return attribution.integrated_gradients(m, x, 1, base, steps=steps, max_batch=B)

    t = rounds({"integrated_gradients": whole, f"{S} saliency steps alone": alone}, a.calls, a.rounds)
    w, f = statistics.median(t["integrated_gradients"]), statistics.median(t[f"{S} saliency steps alone"])
    report(lines, "one encoder (max_batch = B: one path point per forward):", t,
           f"the call costs its {S} forward + data-gradient passes plus {(w - f) / 1e3:.2f} ms = {100 * (w - f) / w:.1f} % of the whole")

    # ---------------------------------------------------------------------------------- the three kernels against torch
    al, wt = (torch.tensor(v, dtype=torch.float32).to(dev) for v in attribution.path_table(steps, "trapezoid"))
    al_h, wt_h = al.tolist(), wt.tolist()
    grad = torch.randn(B, 3, H, H, generator=g).to(dev)
    bimg = base.view(1, 3, 1, 1).expand_as(x).contiguous()

    def hip_kernels():
        acc = torch.zeros_like(x)
        for s in range(S):
            attribution.attr_inputs(x, base, al[s:s + 1])
            attribution.attr_accumulate(grad.view(1, *grad.shape), wt[s:s + 1], acc)
        return attribution.attr_finish(acc, x, base, False, True)

    point = torch.empty_like(x)

    def torch_kernels():
        acc = torch.zeros_like(x)
        for s in range(S):
            torch.lerp(bimg, x, al_h[s], out=point)
            acc.add_(grad, alpha=wt_h[s])
        t_ = acc.mul(x - bimg)
        px = t_.sum(1)
        return F.avg_pool2d(px.unsqueeze(1), 16).squeeze(1) * 256, px, t_.double().sum(dim=(1, 2, 3))

    hm, hp, ht = hip_kernels()
    tm, tp, tt = torch_kernels()
    for name, u, v in (("maps", hm, tm), ("pixels", hp, tp), ("total", ht, tt)):
        e = float((u.double() - v.double()).abs().max() / v.double().abs().max())
        assert e < 1e-5, (name, e)
    moved = (S * 2 + S * 3 + 2 + 1 / 3) * x.numel() * 4          # per step: read x, write the point; read g, read and write acc; finish: acc, x, pixels
    t = rounds({"attr_inputs/accumulate/finish": hip_kernels, "torch composition": torch_kernels}, a.calls * 5, a.rounds)
    m_h, m_t = statistics.median(t["attr_inputs/accumulate/finish"]), statistics.median(t["torch composition"])
    report(lines, f"the three kernels of such a call ({S} x inputs, {S} x accumulate, 1 x finish with the pixel map) against torch:", t,
           f"ratio torch / hip {m_t / m_h:.2f}; {moved / 1e6:.0f} MB read or written by the launches -> {moved / m_h / 1e3:.0f} GB/s (hip, {2 * S + 1} launches and a fill; "
           "x and the gradient are re-read every step, so part of that comes from the caches)")

    # ---------------------------------------------------------------------------------- the two-stream model
    import vits_returnftrs as vrf
    fus = importlib.import_module(FUS_MOD)
    torch.manual_seed(0)
    backs = [vrf.vit_small(num_classes=3, depth=a.depth, img_size=H).to(dev).eval() for _ in range(2)]
    model = fus.Fus_CrossViT(backs[0], backs[1]).to(dev).eval()

    def fus_whole():
        return model.integrated_gradients(backs[0], backs[1], x, xe, target=1, steps=steps, max_batch=B)

    def fus_alone():
        with passes_alone(x):
            return model.integrated_gradients(backs[0], backs[1], x, xe, target=1, steps=steps, max_batch=B)

    t = rounds({"Fus_CrossViT.integrated_gradients": fus_whole, f"{S} forward + backward passes": fus_alone}, max(1, a.calls // 2), a.rounds)
    w, f = statistics.median(t["Fus_CrossViT.integrated_gradients"]), statistics.median(t[f"{S} forward + backward passes"])
    report(lines, "Fus_CrossViT.integrated_gradients (both streams along the joint path, max_batch = B):", t,
           f"the call costs its {S} two-stream passes plus {(w - f) / 1e3:.2f} ms = {100 * (w - f) / w:.1f} % of the whole")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
