"""Times of layer-wise CKA between two ViT encoders (mfvit.similarity; csrc/cka.hip) on one GPU (development aid, not the contract bench; no speed
is gated).  vit_small at 224^2, both encoders, tokens = 'all': 2 x 13 hidden states of [B][197 * 384] f32, read in place from the workspaces of
the two evaluation forwards.

  hip    mfvit_gram_centered on both stacks (the Gram launch and its split reduce), then one mfvit_hsic_accumulate (13 x 13 + 13 + 13 outputs).
  torch  the same work with torch ops on the same GPU: the stacks as (13, B, T D) views, h @ h^T (f32, raw - the uncentred Gram the eager route
         gives), and the three HSIC sums of every pair in float64.
  fwd    the two evaluation forwards with saved activations that produce the hidden states.

Device-event time per call.  Windows are sized in time, not in calls: the warm round times a few calls of each version and from then on a
window of that version is as many calls as fill `--window` seconds (0.25 by default: 300 Gram calls, 7,000 HSIC calls at B = 128).  The
versions alternate inside each of `--rounds` rounds, and the median / min / max over the rounds are reported.  Bytes and FLOP are counted from
the shapes (below), not measured.

    python tools/cka_bench.py [--batches 128 256] [--rounds 7] [--window 0.25] [--out profiles/cka_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-feature-vit_amd"))
import torch  # noqa: E402
import vits  # noqa: E402
from mfvit import _lib, similarity  # noqa: E402

PEAK_F32_MATRIX = 155e12     # v_mfma_f32_32x32x2_f32, measured peak
PEAK_HBM = 8.0e12            # spec; about 6.3e12 achievable


def events(f, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def counts(n, k, reps):
    """(bytes, flop) of the Gram launches of `reps` representations, from the shapes: x read once, the partial tiles written and read once, g
    written; 2 n_tile 32 x 32 x k multiply-adds on the upper triangle of tiles."""
    p = (ctypes.c_int32 * 4)()
    assert _lib.lib().mfvit_gram_plan(n, k, p) == 0
    nt = (n + 31) // 32
    tiles = nt * (nt + 1) // 2
    part = reps * p[1] * tiles * 1024 * 4
    return reps * n * k * 4 + 2 * part + reps * n * n * 8, 2.0 * reps * tiles * 1024 * k


def torch_hsic(ga, gb, unbiased=True):
    """The three sums of every (i, j), (i, i), (j, j) in float64 with torch ops."""
    n = ga.shape[-1]
    K, L = ga.double(), gb.double()
    if unbiased:
        eye = torch.eye(n, device=K.device, dtype=torch.bool)
        K, L = K.masked_fill(eye, 0.0), L.masked_fill(eye, 0.0)

    def h(K, L, pairwise):
        rk, rl = K.sum(-1), L.sum(-1)
        if pairwise:
            s1 = torch.einsum("iab,jab->ij", K, L)
            s2 = rk.sum(-1)[:, None] * rl.sum(-1)[None, :]
            s3 = rk @ rl.T
        else:
            s1, s2, s3 = (K * L).sum((-1, -2)), rk.sum(-1) * rl.sum(-1), (rk * rl).sum(-1)
        return (s1 + s2 / ((n - 1) * (n - 2)) - 2.0 / (n - 2) * s3) / (n * (n - 3))
    return h(K, L, True), h(K, K, False), h(L, L, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timing window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cka_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    h = _lib.lib()
    torch.manual_seed(0)
    models = [vits.vit_small(num_classes=3).to(dev).eval() for _ in range(2)]
    lines = [f"layer-wise CKA, vit_small 224^2 (13 hidden states per encoder), tokens = 'all', two encoders, device {torch.cuda.get_device_name(0)}, "
             f"precision {models[0].precision}; device-event ms per call, windows of {a.window} s of device time (calls per window in brackets), "
             f"median [min .. max] of {a.rounds} rounds after one warm round, versions alternating within a round"]
    for B in a.batches:
        xs = [torch.randn(B, 3, 224, 224, device=dev) for _ in range(2)]
        held = [m._rel_forward(x) for m, x in zip(models, xs)]
        views = [m._hidden_view(cfg, ws) for m, (cfg, ws, _) in zip(models, held)]
        R, n, k = views[0].shape[0], B, views[0].shape[2] * views[0].shape[3]
        nbytes = h.mfvit_gram_work_bytes(R, n, k)
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        g = [torch.empty(R, n, n, device=dev, dtype=torch.float64) for _ in range(2)]
        acc = torch.zeros(R * R + 2 * R, device=dev, dtype=torch.float64)
        st = _lib.stream()

        def gram():
            for v, o in zip(views, g):
                _lib.check(h.mfvit_gram_centered(v.data_ptr(), v.stride(0), v.stride(1), R, n, k, o.data_ptr(), work.data_ptr(), nbytes, st), "gram")

        def hsic():
            p = acc.data_ptr()
            _lib.check(h.mfvit_hsic_accumulate(g[0].data_ptr(), R, g[1].data_ptr(), R, n, 1, p, p + 8 * R * R, p + 8 * (R * R + R), st), "hsic")

        flat = [v.flatten(2) for v in views]
        tg = [None, None]

        def torch_gram():
            for i, f in enumerate(flat):
                tg[i] = f @ f.transpose(1, 2)

        def torch_hs():
            return torch_hsic(tg[0], tg[1])

        def forwards():
            for m, x in zip(models, xs):
                cfg, ws, _ = m._rel_forward(x)
                m._release_ws(ws)

        names = ["hip gram (2 x 13 reps)", "torch gram (raw f32 bmm)", "hip hsic (13 x 13)", "torch hsic (float64 ops)", "two evaluation forwards"]
        fns = [gram, torch_gram, hsic, torch_hs, forwards]
        res = {k_: [] for k_ in names}
        calls = {}
        for name, f in zip(names, fns):               # the warm round, which also sizes every version's window
            events(f, 2)
            calls[name] = max(5, int(a.window * 1e3 / events(f, 5)) + 1)
        for r in range(a.rounds):
            for name, f in zip(names, fns):
                res[name].append(events(f, calls[name]))
        # the two routes agree: CKA from the hip sums against CKA from the torch sums (raw Gram, f32: to its cancellation error)
        acc.zero_()
        gram(); hsic()
        ab, aa, bb = acc[:R * R].view(R, R), acc[R * R:R * R + R], acc[R * R + R:]
        cka_hip = ab / torch.sqrt(aa[:, None] * bb[None, :])
        tab, taa, tbb = torch_hsic(tg[0], tg[1])
        cka_t = tab / torch.sqrt(taa[:, None] * tbb[None, :])
        diff = float((cka_hip - cka_t).abs().max())
        by, fl = counts(n, k, 2 * R)
        med = {k_: statistics.median(v) for k_, v in res.items()}
        tg_ms = med[names[0]]
        t_flop, t_byte = fl / PEAK_F32_MATRIX * 1e3, by / PEAK_HBM * 1e3
        bound = "the f32 matrix rate" if t_flop > t_byte else "HBM bandwidth"
        lines.append(f"B = {B}: n = {n}, k = {k}, {2 * R} Gram matrices; counted from the shapes: {by / 1e9:.3f} GB moved, {fl / 1e9:.1f} GFLOP on the upper-triangle tiles")
        for name in names:
            v = res[name]
            lines.append(f"  {name:<28s} {statistics.median(v):9.3f} ms  [{min(v):9.3f} .. {max(v):9.3f}]  ({calls[name]} calls)")
        lines.append(f"  hip gram: {by / tg_ms / 1e9:.2f} TB/s achieved ({by / tg_ms / 1e9 / 8.0 * 100:.0f} % of the 8 TB/s HBM peak), {fl / tg_ms / 1e9:.1f} TF "
                     f"({fl / tg_ms / 1e9 / 155 * 100:.0f} % of the 155 TF f32 matrix peak); least time {t_flop:.3f} ms by FLOP, {t_byte:.3f} ms by bytes: bound by {bound}, "
                     f"{max(t_flop, t_byte) / tg_ms * 100:.0f} % of that bound")
        lines.append(f"  hip gram + hsic = {(med[names[0]] + med[names[2]]):.3f} ms = {(med[names[0]] + med[names[2]]) / med[names[4]] * 100:.1f} % of the two forwards "
                     f"({med[names[4]]:.3f} ms); torch gram + hsic = {(med[names[1]] + med[names[3]]):.3f} ms; max |CKA hip - CKA torch (raw f32 Gram)| = {diff:.2e}")
        for m, (_, ws, _) in zip(models, held):
            m._release_ws(ws)
        del views, flat, tg, g, work, held
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
