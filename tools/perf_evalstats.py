"""Times of the bootstrap counts (mfvit.evalstats.bootstrap_counts; csrc/evalstats.hip) against the two routes a user had before (development aid,
not the contract bench).  The same statistics - weighted confusion matrices and AUC pair counts of R replicates for M score sets - three ways:

  hip       bootstrap_counts: every (model, class) column ordered once, then O(n) per replicate and column.
  gathered  per replicate a resampled batch (index_select on the device) and one mfvit_eval_counts per score set: R M calls, each an O(n^2) pair
            count - all the library offered before.
  sklearn   scores copied to the host once, then per replicate confusion_matrix per score set and roc_auc_score per score set and class with
            sample_weight (the host loop around the reference's evaluation code).

Wall time per whole run, every round closed by a device synchronisation, warm (one untimed run first), median of the rounds; a round of the
hip path is 50 runs, so that the window is not a fraction of a millisecond.

    python tools/perf_evalstats.py [--n 4096] [--classes 3] [--models 3] [--boot 2000] [--rounds 5] [--host-rounds 3] [--out profiles/evalstats_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mfvit import evalstats, metrics  # noqa: E402


def timed(f, n_rounds, calls=1):
    """ms per run of every round; `calls` runs per round where one run is too short a window"""
    f()                                                                  # warm
    torch.cuda.synchronize()
    out = []
    for _ in range(n_rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--models", type=int, default=3)
    ap.add_argument("--boot", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, C, M, R = a.n, a.classes, a.models, a.boot
    rng = np.random.Generator(np.random.PCG64(0))
    p = np.arange(C, 0, -1, dtype=np.float64)
    labels = rng.choice(C, size=n, p=p / p.sum()).astype(np.int64)
    scores = rng.standard_normal((M, n, C)).astype(np.float32)
    scores[:, np.arange(n), labels] += 1.0
    sd, ld = torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev)

    def hip():
        return evalstats.bootstrap_counts(sd, ld, R, seed=1)

    gen = torch.Generator(device=dev)

    def gathered():
        gen.manual_seed(1)
        out = []
        for _ in range(R):
            idx = torch.randint(n, (n,), device=dev, generator=gen)
            lab = ld.index_select(0, idx)
            for m in range(M):
                conf, _, u2, npos = metrics.eval_counts(sd[m].index_select(0, idx), lab)
                out.append((conf, u2, npos))
        return out

    def sklearn_loop():
        from sklearn.metrics import confusion_matrix, roc_auc_score
        s, t = sd.cpu().numpy().astype(np.float64), ld.cpu().numpy()
        preds = s.argmax(2)
        g = np.random.Generator(np.random.PCG64(1))
        out = []
        for _ in range(R):
            w = np.bincount(g.integers(0, n, size=n), minlength=n)
            for m in range(M):
                out.append(confusion_matrix(t, preds[m], labels=list(range(C)), sample_weight=w))
                for c in range(C):
                    out.append(roc_auc_score(t == c, s[m, :, c], sample_weight=w))
        return out

    # replicate 0 of the new path is the old path's answer on the sample itself
    conf, u2, npos = hip()
    for m in range(M):
        econf, _, eu2, enpos = metrics.eval_counts(sd[m], ld)
        assert torch.equal(conf[0, m], econf) and torch.equal(u2[0, m], eu2) and torch.equal(npos[0], enpos)
    lines = [f"bootstrap counts: n = {n}, C = {C}, M = {M} score sets, R = {R} replicates (+ the sample itself), device "
             f"{torch.cuda.get_device_name(0)}; wall time per whole run, warm"]
    res = {"hip  bootstrap_counts": timed(hip, a.rounds, calls=50), "gathered eval_counts x R M": timed(gathered, a.host_rounds),
           "sklearn loop on the host": timed(sklearn_loop, a.host_rounds)}
    for k, t in res.items():
        lines.append(f"  {k:<28s} median {statistics.median(t):12.2f} ms   min {min(t):12.2f}   max {max(t):12.2f}   ({len(t)} rounds)")
    med = {k: statistics.median(t) for k, t in res.items()}
    h = med["hip  bootstrap_counts"]
    lines.append(f"  ratio gathered / hip {med['gathered eval_counts x R M'] / h:.0f}, sklearn / hip {med['sklearn loop on the host'] / h:.0f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
