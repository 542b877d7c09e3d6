"""Times of the operating points, the curve counts and the calibration sums (mfvit.evalstats; csrc/evalstats.hip) against the routes a user had
before, and the measured accuracy of the device's double exp / log that the calibration test's gate rests on (development aid, not the contract
bench).  The same table - sensitivity / specificity / PPV / NPV at Q operating points of R bootstrap replicates for M score sets and C classes,
and a ROC band over a grid of specificities - three ways:

  hip       operating_points / roc_band: every column ordered once, one workgroup per (replicate, column), a request is a bisection in LDS.
  sklearn   scores on the host, per replicate and column sklearn.metrics.roc_curve with sample_weight (drop_intermediate=False), the points
            read off fps / tps with numpy.
  parent    what the library offered before this kernel: bootstrap_counts on the device for the replicates' AUC and class counts, and for the
            thresholds a resampled batch gathered on the device (index_select), copied to the host and cut with numpy sorts, per replicate.

Wall time per whole run, every round closed by a device synchronisation, warm (one untimed run first), median of the rounds; a round of a short
device path is `--calls` runs, so that the window is not a fraction of a millisecond.  Needs a GPU: there is no fallback.

    python tools/perf_opcurve.py [--n 4096] [--classes 3] [--models 3] [--boot 2000] [--rounds 5] [--host-rounds 1] [--out profiles/opcurve_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mfvit import evalstats  # noqa: E402

U = 2.0 ** -53


def timed(f, n_rounds, calls=1):
    f()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def points_from_curve(fps, tps, P, N, caps, needs):
    """the operating points of one weighted curve (highest threshold first, (0, 0) in front): lowest threshold with fps <= cap, highest with
    tps >= need"""
    out = []
    for cap in caps:
        j = np.nonzero(fps <= cap)[0].max()
        out.append((tps[j], fps[j]))
    for need in needs:
        ok = np.nonzero(tps >= need)[0]
        j = ok.min() if ok.size else len(tps) - 1
        out.append((tps[j], fps[j]))
    return out


def single_row_error(dev):
    """mfvit_calib_sums with ONE row per workgroup (n = 1: no summation, every output is a single term) against the float64 restatement of
    tests/opcurve_ref.py, in units of the double unit roundoff: the worst |device - restatement| / (1 + the magnitude of the term's parts) over
    the three sums, and the worst relative error of the confidence.  The 1 stands for the part of a row's error that does not shrink with the
    term: log(den) near den = 1 and (p_y - 1)^2 near p_y = 1 carry the ABSOLUTE rounding of den and p_y, whatever is left after the cancellation."""
    import opcurve_ref as O
    rng = np.random.Generator(np.random.PCG64(0))
    temps = np.float32(0.05 * 1.49 ** np.arange(16))
    worst, rows = 0.0, 0
    for C in (2, 3, 5, 64):
        for scale in (0.5, 3.0, 20.0):
            for _ in range(40):
                z = (scale * rng.standard_normal((8, 1, C))).astype(np.float32)
                y = rng.integers(0, C, 1).astype(np.int64)
                ref = O.calib_sums(z, y, temps, 15)
                got = evalstats.calib_sums(torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev), temps, 15)
                sums, conf = got[3].cpu().numpy(), got[2].cpu().numpy().sum(2)
                e = np.abs(sums - ref["sums"]) / (1.0 + ref["abs_sums"])
                ec = np.abs(conf - ref["conf"][:, :, 0]) / ref["conf"][:, :, 0]
                worst = max(worst, float(e.max()), float(ec.max()))
                rows += 8 * 16
    return worst / U, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--models", type=int, default=3)
    ap.add_argument("--boot", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_opcurve.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    n, C, M, R = a.n, a.classes, a.models, a.boot
    rng = np.random.Generator(np.random.PCG64(0))
    p = np.arange(C, 0, -1, dtype=np.float64)
    labels = rng.choice(C, size=n, p=p / p.sum()).astype(np.int64)
    scores = rng.standard_normal((M, n, C)).astype(np.float32)
    scores[:, np.arange(n), labels] += 1.0
    sd, ld = torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev)
    at = [("specificity", 0.95), ("sensitivity", 0.9), ("threshold", 0.5)]
    grid = [k / 20 for k in range(21)]
    req, req_band = evalstats.encode_requests(at), evalstats.encode_requests([("specificity", g) for g in grid])

    def host_requests(P, N):
        caps = [(int(r[1]) * N) // int(r[2]) for r in np.concatenate([req, req_band]) if r[0] == 0]
        needs = [-((-int(r[1]) * P) // int(r[2])) for r in req if r[0] == 1]
        return caps, needs

    def sklearn_loop():
        from sklearn.metrics import roc_curve
        s, t = sd.cpu().numpy().astype(np.float64), ld.cpu().numpy()
        g = np.random.Generator(np.random.PCG64(1))
        out = []
        for _ in range(R + 1):
            w = np.bincount(g.integers(0, n, size=n), minlength=n).astype(np.float64)
            for c in range(C):
                y = t == c
                P = int(w[y].sum())
                if P == 0 or P == n:
                    continue
                caps, needs = host_requests(P, n - P)
                for m in range(M):
                    keep = w > 0
                    fpr, tpr, thr = roc_curve(y[keep], s[m, keep, c], sample_weight=w[keep], drop_intermediate=False)
                    out.append(points_from_curve(np.rint(fpr * (n - P)), np.rint(tpr * P), P, n - P, caps, needs))
                    out.append(((w * y * (s[m, :, c] >= 0.5)).sum(), (w * ~y * (s[m, :, c] >= 0.5)).sum()))
        return out

    gen = torch.Generator(device=dev)

    def parent_route():
        evalstats.bootstrap_counts(sd, ld, R, seed=1)
        gen.manual_seed(1)
        t = ld.cpu().numpy()
        out = []
        for _ in range(R + 1):
            idx = torch.randint(n, (n,), device=dev, generator=gen)
            s = sd.index_select(1, idx).cpu().numpy()
            tr = t[idx.cpu().numpy()]
            for c in range(C):
                y = tr == c
                P = int(y.sum())
                if P == 0 or P == n:
                    continue
                caps, needs = host_requests(P, n - P)
                for m in range(M):
                    order = np.argsort(-s[m, :, c], kind="stable")
                    ys, ss = y[order], s[m, order, c]
                    last = np.r_[np.nonzero(np.diff(ss))[0], n - 1]
                    tps, fps = np.r_[0, np.cumsum(ys)[last]], np.r_[0, np.cumsum(~ys)[last]]
                    out.append(points_from_curve(fps, tps, P, n - P, caps, needs))
                    out.append(((y & (s[m, :, c] >= 0.5)).sum(), (~y & (s[m, :, c] >= 0.5)).sum()))
        return out

    lines = [f"operating points: n = {n}, C = {C}, M = {M} score sets, R = {R} replicates (+ the sample itself), {len(at)} requests and a "
             f"{len(grid)}-point ROC band, device {torch.cuda.get_device_name(0)}; wall time per whole run, warm"]
    res = {
        "hip  bootstrap_points, 3 requests (device counts)": timed(lambda: evalstats.bootstrap_points(sd, ld, req, R, seed=1), a.rounds, a.calls),
        "hip  bootstrap_points, 21-point band (device counts)": timed(lambda: evalstats.bootstrap_points(sd, ld, req_band, R, seed=1), a.rounds, a.calls),
        "hip  operating_points (+ copy, host intervals)": timed(lambda: evalstats.operating_points(sd, ld, at, R, seed=1), a.rounds),
        "hip  roc_band (+ copy, host intervals)": timed(lambda: evalstats.roc_band(sd, ld, grid, R, seed=1), a.rounds),
        "hip  curve_counts": timed(lambda: evalstats.curve_counts(sd, ld), a.rounds, a.calls),
        "hip  calib_sums, 1 temperature, 15 bins": timed(lambda: evalstats.calib_sums(sd, ld, [1.0], 15), a.rounds, a.calls),
        "hip  calib_sums, 16 temperatures, 15 bins": timed(lambda: evalstats.calib_sums(sd, ld, np.float32(0.25 * 1.3 ** np.arange(16)), 15), a.rounds, a.calls),
        "hip  fit_temperature (one score set)": timed(lambda: evalstats.fit_temperature(sd[0], ld), a.rounds),
        "parent: bootstrap_counts + gathered scores, numpy": timed(parent_route, a.host_rounds),
        "sklearn roc_curve loop on the host (points + band)": timed(sklearn_loop, a.host_rounds),
    }
    for k, t in res.items():
        lines.append(f"  {k:<54s} median {statistics.median(t):12.3f} ms   min {min(t):12.3f}   max {max(t):12.3f}   ({len(t)} rounds)")
    med = {k: statistics.median(t) for k, t in res.items()}
    both = med["hip  operating_points (+ copy, host intervals)"] + med["hip  roc_band (+ copy, host intervals)"]
    lines.append(f"  ratio to operating_points + roc_band: parent route {med['parent: bootstrap_counts + gathered scores, numpy'] / both:.0f}, "
                 f"sklearn loop {med['sklearn roc_curve loop on the host (points + band)'] / both:.0f}")
    worst, rows = single_row_error(dev)
    lines.append(f"calibration, accuracy of the device's double exp / log / divide: worst single-row error {worst:.2f} U (U = 2^-53) over {rows} "
                 f"(row, temperature) terms, against numpy float64 (mfvit_calib_sums with n = 1: no summation; sums: |error| / (1 + magnitude of "
                 f"the term's parts), confidence: relative)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
