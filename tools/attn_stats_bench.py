"""Times of the per-head attention statistics (mfvit.attnstats; csrc/attention_maps.hip, attn_stats_kernel) on one GPU (development aid, not the
contract bench; no speed is gated).  vit_small at 224^2, both encoders, all 12 blocks, B = 128 by default.

  stats  mfvit_attention_stats on the workspaces of two evaluation forwards with saved activations: one launch over the 12 blocks of an
         encoder (B * 12 * 12 * 7 workgroups) and its finish launch, per encoder.
  maps   the route it replaces: get_attention_maps(x) (its own evaluation forward plus 12 per-head map launches: 12 x B x 12 x 197 x 197 f32
         written to HBM) and the six statistics from those maps with torch ops, per encoder.
  fwd    the two evaluation forwards with saved activations.

Device-event time per call; one warm round, then the versions alternate inside each of `--rounds` rounds; median [min .. max] over the rounds.

    python tools/attn_stats_bench.py [--batch 128] [--rounds 5] [--out profiles/attn_stats_bench.txt]
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
from mfvit import _lib, attnstats  # noqa: E402


def events(f, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_stats(P, d):
    """The six statistics of (B, H, T, T) f32 maps with torch ops (f32 products, float64 sums over the rows): (B, H, 6)."""
    T = P.shape[-1]
    Pp = P[..., 1:, 1:]
    pd = (Pp * d).sum(-1)
    H = torch.special.entr(P).sum(-1)
    return torch.stack([pd.double().mean(-1), (pd / Pp.sum(-1)).double().mean(-1), H.double().mean(-1), H[..., 0].double(),
                        P[..., 1:, 0].double().mean(-1), torch.diagonal(P, dim1=-2, dim2=-1).double().mean(-1)], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_stats_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    h = _lib.lib()
    torch.manual_seed(0)
    B, T, H, L, hd = a.batch, 197, 12, 12, 32
    models = [vits.vit_small(num_classes=3).to(dev).eval() for _ in range(2)]
    xs = [torch.randn(B, 3, 224, 224, device=dev) for _ in range(2)]
    held = [m._rel_forward(x) for m, x in zip(models, xs)]
    out = (ctypes.c_int64 * 4)()
    _lib.check(h.mfvit_vit_attn_layout(held[0][0], out), "layout")
    nbytes = h.mfvit_attention_stats_work_bytes(L, B, T, H)
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    res_hip = [torch.empty(L, B, H, 6, device=dev, dtype=torch.float64) for _ in range(2)]
    st = _lib.stream()
    i = torch.arange(T - 1, device=dev)
    yx = torch.stack([i // 14, i % 14], dim=1).float()
    d = 16.0 * torch.cdist(yx, yx)

    def stats():
        for (cfg, ws, _), o in zip(held, res_hip):
            p = ws.data_ptr()
            _lib.check(h.mfvit_attention_stats(out[3], p + out[0], p + out[1], out[2], out[2], L, B, T, H, hd, 14, 14, 16.0, o.data_ptr(),
                                               work.data_ptr(), nbytes, st), "stats")

    res_t = [None, None]

    def maps_route():
        for k, (m, x) in enumerate(zip(models, xs)):
            res_t[k] = torch.stack([torch_stats(P, d) for P in m.get_attention_maps(x)])

    def forwards():
        for m, x in zip(models, xs):
            cfg, ws, _ = m._rel_forward(x)
            m._release_ws(ws)

    def full():
        for m, x in zip(models, xs):
            m.attention_stats(x)

    names = ["stats launches (2 encoders x 12 blocks)", "attention_stats(x) x 2 (forward + launch)", "maps route x 2 (get_attention_maps + torch)",
             "two evaluation forwards (saved)"]
    fns = [stats, full, maps_route, forwards]
    calls = {}
    for name, f in zip(names, fns):               # the warm round, which also sizes every version's window
        events(f, 1)
        calls[name] = max(3, min(200, int(250.0 / events(f, 2)) + 1))
    res = {n: [] for n in names}
    for r in range(a.rounds):
        for name, f in zip(names, fns):
            res[name].append(events(f, calls[name]))
    stats()
    maps_route()
    diff = max(float(((g - t).abs() / (t.abs() + torch.tensor([16.0, 16.0, 1, 1, 1, 1], device=dev, dtype=torch.float64))).max()) for g, t in zip(res_hip, res_t))
    med = {n: statistics.median(v) for n, v in res.items()}
    maps_bytes = 2 * L * B * H * T * T * 4
    flop = 2.0 * 2 * L * B * H * (7 * 32) * (7 * 32) * hd
    lines = [f"per-head attention statistics, vit_small 224^2, both encoders, 12 blocks each, B = {B}, device {torch.cuda.get_device_name(0)}, precision "
             f"{models[0].precision} (qkv storage tag {out[3]}); device-event ms per call, median [min .. max] of {a.rounds} rounds after one warm round, "
             "versions alternating within a round"]
    for name in names:
        v = res[name]
        lines.append(f"  {name:<46s} {statistics.median(v):9.3f} ms  [{min(v):9.3f} .. {max(v):9.3f}]  ({calls[name]} calls)")
    s_ms, f_ms, m_ms, a_ms = med[names[0]], med[names[3]], med[names[2]], med[names[1]]
    lines.append(f"  stats launches = {s_ms / f_ms * 100:.1f} % of the two forwards they follow; {flop / s_ms / 1e9:.1f} TF on the padded score tiles "
                 f"(f32 MFMA, {flop / s_ms / 1e9 / 155 * 100:.0f} % of the 155 TF f32 matrix peak)")
    lines.append(f"  maps route / attention_stats(x), both with their forwards: {m_ms / a_ms:.1f} x;  (maps route - two forwards) / stats launches: "
                 f"{(m_ms - f_ms) / s_ms:.1f} x;  the maps route writes {maps_bytes / 1e9:.2f} GB of per-head maps and reads them back")
    lines.append(f"  largest |stats - torch on the maps| / (|ref| + scale) = {diff:.2e} (the torch route sums rows in f32)")
    for m, (_, ws, _) in zip(models, held):
        m._release_ws(ws)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
