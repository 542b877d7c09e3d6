"""Times of the perturbation test for relevance maps (mfvit.perturb; csrc/perturb.hip) against the torch composition it replaces and against
the model forwards it cannot avoid (development aid, not the contract bench).  Three measurements, each in interleaved rounds on one GPU with
device events (ours, theirs, ours, theirs ...), median and spread of the rounds:

  mask    patch_rank + perturb_patches (two launches) at B images of size^2, S steps of positive perturbation, against the torch
          composition: a per-image argsort once, then per step a scatter into a patch mask, an upsample and a where into the same
          preallocated (S, B, C, H, W) output.  Same inputs, results compared bit for bit before the timing.
  score   perturb_score (one launch) against softmax in double, gather, argmax and the sums in torch, accumulated into tensors.
  test    Fus_CrossViT.perturbation_test of the two-stream model (both streams perturbed, max_batch = B) against the S evaluation forwards
          alone on batches masked beforehand; the share of the whole test that is not the forwards.

    python tools/perf_perturb.py [--batch 64] [--size 224] [--steps 10] [--depth 12] [--calls 20] [--rounds 5] [--out profiles/perturb_bench.txt]
"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
from mfvit import perturb  # noqa: E402

FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def rounds(impls, calls, n_rounds, warmup=3):
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
        lines.append(f"  {k:<28s} median {statistics.median(t):10.1f} us   min {min(t):10.1f}   max {max(t):10.1f}   ({len(t)} rounds)")
    if extra:
        lines.append("  " + extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, S = a.batch, a.size, a.steps
    gh = H // 16
    P = gh * gh
    g = torch.Generator().manual_seed(0)
    x, xe = torch.randn(B, 3, H, H, generator=g).to(dev), torch.randn(B, 3, H, H, generator=g).to(dev)
    rel = torch.randn(B, P, generator=g).to(dev)
    ks = perturb.step_counts(P, [s / S for s in range(S)])
    ranges = perturb.ranges_for(P, ks, "positive")
    r_dev = ranges.to(dev)
    lines = [f"perturbation test: B = {B}, {H} x {H}, P = {P}, S = {S} steps (k = {ks}), device {torch.cuda.get_device_name(0)}"]

    # ---------------------------------------------------------------------------------- mask
    def hip_mask():
        return perturb.perturb_patches(x, perturb.patch_rank(rel), r_dev)

    out_t = torch.empty(S, B, 3, H, H, device=dev)
    zero = torch.zeros((), device=dev)

    def torch_mask():
        order = torch.argsort(rel, dim=1, descending=True, stable=True)
        for s, k in enumerate(ks):
            mask = torch.zeros(B, P, device=dev, dtype=torch.bool)
            mask.scatter_(1, order[:, :k], True)
            pix = mask.view(B, 1, gh, gh).repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)
            torch.where(pix, zero, x, out=out_t[s])
        return out_t

    assert torch.equal(hip_mask(), torch_mask())
    moved = (1 + S) * x.numel() * 4
    t = rounds({"patch_rank + perturb_patches": hip_mask, "torch composition": torch_mask}, a.calls, a.rounds)
    m_h, m_t = statistics.median(t["patch_rank + perturb_patches"]), statistics.median(t["torch composition"])
    report(lines, "mask path (all S masked batches from the relevance map):", t,
           f"ratio torch / hip {m_t / m_h:.2f}; {moved / 1e6:.1f} MB read once and written S times -> {moved / m_h / 1e3:.0f} GB/s (hip, rank launch included)")

    # ---------------------------------------------------------------------------------- score
    C = 3
    logits = torch.randn(S, B, C, generator=g).to(dev) * 3
    target = torch.randint(0, C, (B,), generator=g).to(dev)
    correct, sums, nonfinite = (torch.zeros(S, dtype=torch.int64, device=dev), torch.zeros(S, 2, dtype=torch.float64, device=dev),
                                torch.zeros(S, dtype=torch.int64, device=dev))
    c_t, s_t = torch.zeros(S, dtype=torch.int64, device=dev), torch.zeros(S, 2, dtype=torch.float64, device=dev)
    idx = target.view(1, B, 1).expand(S, B, 1)

    def hip_score():
        perturb.perturb_score(logits, target, correct, sums, nonfinite)

    def torch_score():
        z = logits.double()
        s_t[:, 0] += z.softmax(dim=2).gather(2, idx).sum(dim=(1, 2))
        s_t[:, 1] += z.gather(2, idx).sum(dim=(1, 2))
        c_t.add_((logits.argmax(dim=2) == target).sum(dim=1))

    hip_score()
    torch_score()
    assert torch.equal(correct, c_t) and float(((sums - s_t).abs() / s_t.abs().clamp_min(1e-30)).max()) < 1e-12
    report(lines, "score (S x B x 3 logits into per-step counts and sums):", rounds({"perturb_score": hip_score, "torch equivalent": torch_score},
                                                                                   a.calls, a.rounds))

    # ---------------------------------------------------------------------------------- the whole test of the two-stream model
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    torch.manual_seed(0)
    backs = [vits.vit_small(num_classes=3, depth=a.depth, img_size=H).to(dev).eval() for _ in range(2)]
    model = fus.Fus_CrossViT(backs[0], backs[1]).to(dev).eval()
    maps = (rel.view(B, gh, gh), rel.flip(1).view(B, gh, gh))
    fr = [s / S for s in range(S)]

    def whole():
        return model.perturbation_test(backs[0], backs[1], x, xe, maps, target=1, fractions=fr, max_batch=B)

    mc = perturb.perturb_patches(x, perturb.patch_rank(maps[0]), r_dev)
    me = perturb.perturb_patches(xe, perturb.patch_rank(maps[1]), r_dev)

    def forwards():
        with torch.no_grad():
            for s in range(S):
                fused, x_c, x_e = model(backs[0], backs[1], mc[s], me[s])
                out = fused + x_c + x_e
        return out

    t = rounds({"perturbation_test": whole, f"{S} forwards alone": forwards}, max(1, a.calls // 10), a.rounds, warmup=2)
    w, f = statistics.median(t["perturbation_test"]), statistics.median(t[f"{S} forwards alone"])
    report(lines, f"Fus_CrossViT.perturbation_test (vit_small depth {a.depth}, both streams perturbed, max_batch = B):", t,
           f"the test costs the {S} forwards plus {(w - f) / 1e3:.2f} ms = {100 * (w - f) / w:.1f} % of the whole")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
