"""Single-kernel parity of the multi-tensor optimizer kernels (csrc/optim.hip) against float64 single steps (oracle/ref_optim.py) on the same
float32 inputs, (a) through hand-built chunk tables over views into NaN-padded flat buffers - every size edge of adam_kernel's float4 / pair /
tail split, every pointer of p / g / m / v off a 16-byte boundary in turn, tensors over several table rows, interleaved rows - and (b) through
mfvit.optim.{Adam, AdamW, SGD} and moco.optimizer.LARS on parameters that are consecutive views of ONE flat arena (mfvit/arena.py), where a
3-element bias shifts everything behind it off alignment, with gradients and states laid out the same way at other phases.
Three steps each, the kernel's own float32 state fed back, so every step is compared on its own.  Gates: the project's own (Adam / AdamW / SGD:
test_adam_parameters_with_different_step_counts_match_torch; LARS: the golden trajectory test), on p and on the states.
tests/test_step_refs_cpu.py pins the references to torch.optim / the reference's LARS and shows that the Adam gate catches a dropped pair
group or tail.  Measured errors are appended to parity_moco_ops.txt (beside the parity_ops.txt of tests/test_ops_gpu.py)
as multiples of the gate."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
NAN = float("nan")
CHUNK_ROW = 1 << 14       # elements per table row, as mfvit.optim lays tables out (asserted below)


def f32(x):
    return float(np.float32(x))   # hyperparameters cross the C ABI as floats: the rounded value is the input


ADAM_RTOL, ADAM_ATOL = 2e-6, 2e-7       # Adam / AdamW / SGD
LARS_RTOL, LARS_ATOL = 5e-6, 1e-7
ADAM_HYPER = dict(lr=f32(1e-2), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), weight_decay=f32(0.1))
ADAM_STEPS = (1, 2, 1000)               # the step number of the first of the three steps


def log(msg):
    from test_ops_gpu import REPORT as OPS_REPORT              # the report directory of the single-op parity tests
    report = os.path.join(os.path.dirname(OPS_REPORT), "parity_moco_ops.txt")
    os.makedirs(os.path.dirname(report), exist_ok=True)
    with open(report, "a") as f:
        f.write(msg + "\n")


def same_bits(a, b, writable=None):
    a, b = a.view(torch.int32), b.view(torch.int32)
    if writable is None:
        return torch.equal(a, b)
    return torch.equal(a[~writable], b[~writable])


class Flat:
    """Views of given sizes inside one NaN-filled flat buffer: each view starts `phase` floats (0..3) behind a 16-byte boundary, at least four
    NaNs lie between two views and PAD around them all.  `mask` marks the views' elements."""

    def __init__(self, counts, phases, values):
        offs, cur = [], PAD
        for c, ph in zip(counts, phases):
            cur = (cur + 3) // 4 * 4 + ph
            offs.append(cur)
            cur += c + 4
        self.buf = torch.full((cur + PAD,), NAN, device=DEV, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.mask = torch.zeros_like(self.buf, dtype=torch.bool)
        self.offs, self.counts = offs, list(counts)
        for o, c, v in zip(offs, counts, values):
            self.buf[o:o + c] = v.to(DEV)
            self.mask[o:o + c] = True

    def view(self, i):
        return self.buf[self.offs[i]:self.offs[i] + self.counts[i]]

    def addr(self, i, a=0):
        return self.buf.data_ptr() + 4 * (self.offs[i] + a)


def phases_for(n, off):
    """Phases of n views: all 0 (aligned) or walking through 1, 2, 3 (every way of being off a boundary)."""
    return [(1 + i % 3) if off else 0 for i in range(n)]


def build_table(order, counts, flats, flags):
    """int64 rows [tensor_id, p, g, s0, s1, count, flag]: `order` lists (tensor, chunk) pairs; flats = (P, G, S0, S1 or None)."""
    rows = []
    for tid, ch in order:
        a = ch * CHUNK_ROW
        c = min(CHUNK_ROW, counts[tid] - a)
        assert c > 0
        rows.append([tid] + [0 if f is None else f.addr(tid, a) for f in flats] + [c, flags[tid]])
    return torch.tensor(rows, dtype=torch.int64).to(DEV)


def chunks_in_order(counts):
    return [(tid, ch) for tid, c in enumerate(counts) for ch in range((c + CHUNK_ROW - 1) // CHUNK_ROW)]


def test_table_rows_are_the_optimizers_chunks():
    from mfvit import optim
    assert optim.CHUNK == CHUNK_ROW and CHUNK_ROW % 4 == 0


# ------------------------------------------------------------------------------------------------ Adam / AdamW through raw tables
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_adam_kernel_size_edges_and_pointer_alignments(decoupled):
    from conftest import rng_tensor
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_optim
    counts = list(ref_optim.ADAM_COUNTS) + [3 * CHUNK_ROW + 5]          # the last tensor: four table rows
    nt = len(counts)
    paths, worst = set(), {}
    for align in ref_optim.ADAM_ALIGN:
        for step0 in ADAM_STEPS:
            vals = {k: [rng_tensor(6000 + 10 * i + j, (c,), scale=s) for i, c in enumerate(counts)]
                    for j, (k, s) in enumerate((("p", 1.0), ("g", 1.0), ("m", 0.1), ("v", 0.1)))}
            vals["v"] = [v.abs() for v in vals["v"]]
            if step0 == 1:
                vals["m"], vals["v"] = [torch.zeros_like(v) for v in vals["m"]], [torch.zeros_like(v) for v in vals["v"]]
            F = {k: Flat(counts, phases_for(nt, align in (k, "all")), vals[k]) for k in "pgmv"}
            table = build_table(chunks_in_order(counts), counts, [F[k] for k in "pgmv"], [int(decoupled)] * nt)
            for row in table.tolist():
                aligned = all(a % 16 == 0 for a in row[1:5])
                assert aligned == (align == "aligned")
                paths |= {(aligned, int(x)) for x in set(ref_optim.adam_path_of(row[5], aligned).tolist())}
            for s in range(3):
                before = {k: F[k].buf.clone() for k in "pgmv"}
                check(lib().mfvit_adam_step(ptr(table), table.shape[0], ADAM_HYPER["lr"], ADAM_HYPER["beta1"], ADAM_HYPER["beta2"], ADAM_HYPER["eps"],
                                            ADAM_HYPER["weight_decay"], step0 + s, stream()), "mfvit_adam_step")
                torch.cuda.synchronize()
                ref = ref_optim.adam_step(*[before[k][F[k].mask] for k in "pgmv"], step0 + s, decoupled=decoupled, **ADAM_HYPER)
                assert same_bits(F["g"].buf, before["g"])
                for k, r in zip("pmv", ref):
                    assert same_bits(F[k].buf, before[k], F[k].mask), (align, step0, s, k)         # the NaNs between and around the views
                    e = ref_optim.gate_ratio(F[k].buf[F[k].mask], r, ADAM_RTOL, ADAM_ATOL)
                    worst[k] = max(worst.get(k, 0.0), e)
                    assert e <= 1.0, (align, step0, s, k, e)
                F["g"].buf.mul_(-0.7)                                   # another gradient for the next step
    log(f"adam_kernel[{'AdamW' if decoupled else 'Adam'}, {len(counts)} tensors x 6 alignments x first step in {ADAM_STEPS} x 3 steps] "
        + " ".join(f"{k} {v:.2f}" for k, v in worst.items()) + f"  of the gate rtol {ADAM_RTOL:.0e} atol {ADAM_ATOL:.0e}")
    # every path of the kernel ran: float4 group without a partner, float4 pair, scalar tail (aligned rows), all-scalar fallback (any pointer off)
    assert paths == {(True, 0), (True, 1), (True, 2), (False, 3)}, paths


# ------------------------------------------------------------------------------------------------ SGD through raw tables
@pytest.mark.parametrize("momentum,wd", [(0.9, 0.0), (0.9, 0.01), (0.0, 0.0), (0.0, 0.01)])
@pytest.mark.parametrize("first", [1, 0])
def test_sgd_kernel_first_step_momentum_and_weight_decay(first, momentum, wd):
    from conftest import rng_tensor
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_optim
    counts = [1, 3, 5, 255, 256, 257, 1153, CHUNK_ROW + 7]
    nt = len(counts)
    lr, mom, wd = f32(0.1), f32(momentum), f32(wd)
    worst = 0.0
    for align in ("aligned", "p", "g", "m", "all"):
        vals = {k: [rng_tensor(6500 + 10 * i + j, (c,)) for i, c in enumerate(counts)] for j, k in enumerate("pgm")}
        F = {k: Flat(counts, phases_for(nt, align in (k, "all")), vals[k]) for k in "pgm"}
        # momentum == 0: the kernel must not touch the state at all - its column of the table is a null pointer
        table = build_table(chunks_in_order(counts), counts, [F["p"], F["g"], F["m"] if mom else None, None], [0] * nt)
        for s in range(3):
            before = {k: F[k].buf.clone() for k in "pgm"}
            fs = first and s == 0
            check(lib().mfvit_sgd_step(ptr(table), table.shape[0], lr, mom, wd, int(fs), stream()), "mfvit_sgd_step")
            torch.cuda.synchronize()
            r_p, r_b = ref_optim.sgd_step(before["p"][F["p"].mask], before["g"][F["g"].mask], before["m"][F["m"].mask], lr, mom, wd, first_step=fs)
            assert same_bits(F["g"].buf, before["g"]) and same_bits(F["p"].buf, before["p"], F["p"].mask)
            if mom:
                assert same_bits(F["m"].buf, before["m"], F["m"].mask)
                e = ref_optim.gate_ratio(F["m"].buf[F["m"].mask], r_b, ADAM_RTOL, ADAM_ATOL)
            else:
                assert same_bits(F["m"].buf, before["m"])
                e = 0.0
            e = max(e, ref_optim.gate_ratio(F["p"].buf[F["p"].mask], r_p, ADAM_RTOL, ADAM_ATOL))
            worst = max(worst, e)
            assert e <= 1.0, (align, s, e)
            F["g"].buf.mul_(-0.7)
    log(f"sgd_kernel[first_step={first}, momentum={momentum}, wd={wd:g}, 5 alignments x 3 steps] {worst:.2f} of the gate rtol {ADAM_RTOL:.0e} atol {ADAM_ATOL:.0e}")


# ------------------------------------------------------------------------------------------------ LARS through raw tables
def test_lars_kernels_norms_over_table_rows_and_tensor_routing():
    """Tensor 0 spans four table rows and tensor 4 two, their rows interleaved with each other's and with the other tensors': the norms are
    summed per tensor_id across rows, wherever the rows stand.  Tensor 1 is 1-D (flag 0: no trust ratio, no weight decay), tensor 2 a zero
    parameter (q = 1), tensor 3 gets the gradient -wd * p at the second step (zero update norm, q = 1; wd is a power of two, so it cancels exactly)."""
    from conftest import rng_tensor
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_optim
    counts = [3 * CHUNK_ROW + 5, 37, 1153, 515, CHUNK_ROW + 3]
    flags = [1, 0, 1, 1, 1]
    order = [(0, 0), (4, 0), (1, 0), (0, 1), (2, 0), (4, 1), (0, 2), (3, 0), (0, 3)]
    assert sorted(order) == chunks_in_order(counts)
    nt = len(counts)
    lr, wd, mom, trust = f32(0.3), 2.0 ** -6, f32(0.9), f32(0.001)
    worst = 0.0
    for align in ("aligned", "p", "g", "m", "all"):
        vals = {k: [rng_tensor(6800 + 10 * i + j, (c,), scale=0.1 if k == "m" else 1.0) for i, c in enumerate(counts)] for j, k in enumerate("pgm")}
        vals["p"][2] = torch.zeros(counts[2])
        F = {k: Flat(counts, phases_for(nt, align in (k, "all")), vals[k]) for k in "pgm"}
        table = build_table(order, counts, [F["p"], F["g"], F["m"], None], flags)
        nbuf = torch.full((PAD + 2 * nt + PAD,), NAN, device=DEV)
        norms = nbuf[PAD:PAD + 2 * nt]
        for s in range(3):
            if s == 1:
                F["g"].view(3).copy_(-wd * F["p"].view(3))
            before = {k: F[k].buf.clone() for k in "pgm"}
            check(lib().mfvit_lars_step(ptr(table), table.shape[0], nt, ptr(norms), lr, wd, mom, trust, stream()), "mfvit_lars_step")
            torch.cuda.synchronize()
            assert same_bits(F["g"].buf, before["g"])
            assert bool(torch.isnan(nbuf[:PAD]).all()) and bool(torch.isnan(nbuf[PAD + 2 * nt:]).all())
            for k in "pm":
                assert same_bits(F[k].buf, before[k], F[k].mask), (align, s, k)
            for i in range(nt):
                sl = {k: slice(F[k].offs[i], F[k].offs[i] + counts[i]) for k in "pgm"}
                r_p, r_m = ref_optim.lars_step(before["p"][sl["p"]], before["g"][sl["g"]], before["m"][sl["m"]], lr, wd, mom, trust, ndim=2 if flags[i] else 1)
                e = max(ref_optim.gate_ratio(F["p"].view(i), r_p, LARS_RTOL, LARS_ATOL), ref_optim.gate_ratio(F["m"].view(i), r_m, LARS_RTOL, LARS_ATOL))
                worst = max(worst, e)
                assert e <= 1.0, (align, s, i, e)
                if flags[i]:            # the norms the update used: |p|^2 and |g + wd p|^2 of the whole tensor
                    pd = before["p"][sl["p"]].double()
                    ud = before["g"][sl["g"]].double() + wd * pd
                    for got, want in ((norms[2 * i], pd.square().sum()), (norms[2 * i + 1], ud.square().sum())):
                        assert abs(float(got) - float(want)) <= 5e-6 * float(want), (align, s, i)
            if s == 1:
                assert float(norms[2 * 3 + 1]) == 0.0                  # the cancelled update: its norm is exactly 0
            F["g"].buf.mul_(-0.7)
    log(f"lars kernels[5 tensors in 9 interleaved rows, 5 alignments x 3 steps] {worst:.2f} of the gate rtol {LARS_RTOL:.0e} atol {LARS_ATOL:.0e}")


# ------------------------------------------------------------------------------------------------ mfvit_amp_unscale
def test_amp_unscale_flag_at_every_position_and_never_cleared():
    from conftest import rng_tensor
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_optim
    counts = [CHUNK_ROW, CHUNK_ROW, 1027]                               # three rows; the last one ends in the 3 elements behind its float4 groups
    inv = 2.0 ** -12                                                    # a power of two: g * inv_scale is exact in float32
    places = {"first element of the first row": (0, 0), "last element of the first row": (0, CHUNK_ROW - 1),
              "4th wave of the middle row": (1, 256 * 5 + 200), "the last row's tail": (2, 1026)}
    assert 192 <= places["4th wave of the middle row"][1] % 256 < 256

    def run(plant=None, flag0=0.0, big=None):
        vals = [rng_tensor(6900 + i, (c,), scale=100.0) for i, c in enumerate(counts)]
        if plant is not None:
            vals[plant[0]][plant[1]] = plant[2]
        if big is not None:
            vals[1][77], vals[2][1025] = big, -big
        G = Flat(counts, [0, 2, 1], vals)
        P = Flat(counts, [0, 0, 0], vals)
        table = build_table(chunks_in_order(counts), counts, [P, G, None, None], [0] * 3)
        fbuf = torch.full((PAD + 1 + PAD,), NAN, device=DEV)
        fbuf[PAD] = flag0
        g0, p0 = G.buf.clone(), P.buf.clone()
        check(lib().mfvit_amp_unscale(ptr(table), table.shape[0], inv, ptr(fbuf[PAD:]), stream()), "mfvit_amp_unscale")
        torch.cuda.synchronize()
        assert same_bits(P.buf, p0) and same_bits(G.buf, g0, G.mask)
        assert bool(torch.isnan(fbuf[:PAD]).all()) and bool(torch.isnan(fbuf[PAD + 1:]).all())
        want, found = ref_optim.amp_unscale(g0[G.mask], inv)
        got = G.buf[G.mask]
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(got)].double(), want[~torch.isnan(want)])   # bit-exact
        return float(fbuf[PAD]), found

    assert run() == (0.0, False)                                        # a clean run leaves 0 at 0 ...
    assert run(flag0=1.0) == (1.0, False)                               # ... and never clears a flag that is set
    assert run(big=float(np.finfo(np.float32).max)) == (0.0, False)     # +-3.4028235e38, the largest finite float, is finite
    n = 0
    for where, (i, j) in places.items():
        for bad in (float("inf"), -float("inf"), float("nan")):
            assert run(plant=(i, j, bad)) == (1.0, True), (where, bad)
            n += 1
    assert run(plant=(1, 5, float("inf")), flag0=1.0) == (1.0, True)
    log(f"amp_unscale[3 table rows, inv_scale 2^-12]: bit-exact, flag set for inf / -inf / nan at {n // 3} positions, never cleared, +-FLT_MAX not flagged")


# ------------------------------------------------------------------------------------------------ the optimizers on one flat arena
ARENA_SHAPES = [(3,), (5,), (1153,), (33, 7), (129, 3), (70000,), (3,), (257, 4), (6,)]     # a 3-class head.bias first: everything behind it is off
FROZEN = 3                                                                                  # this one never gets a gradient


def _arena_setup(opt_name):
    """Parameters as consecutive views of one ParamArena buffer; gradients and optimizer states as consecutive views of NaN-guarded flat
    buffers that start at other phases (2 / 1 / 3 floats behind a boundary)."""
    from conftest import rng_tensor
    from mfvit.arena import ParamArena
    ps = [torch.nn.Parameter(rng_tensor(7100 + i, s).to(DEV)) for i, s in enumerate(ARENA_SHAPES)]
    arena = ParamArena([(f"p{i}", p) for i, p in enumerate(ps)])
    assert arena.intact() and arena.flat.data_ptr() % 16 == 0
    assert {(p.data_ptr() // 4) % 4 for p in ps} == {0, 1, 2, 3}
    total = arena.flat.numel()
    flats = {}
    for j, (name, ph) in enumerate((("grad", 2), ("s0", 1), ("s1", 3))):
        buf = torch.full((PAD + ph + total + PAD,), NAN, device=DEV)
        assert buf.data_ptr() % 16 == 0
        win = buf[PAD + ph:PAD + ph + total]
        win.copy_(rng_tensor(7200 + j, (total,)).to(DEV) if name == "grad" else torch.zeros(total, device=DEV))
        flats[name] = (buf, win, arena.grad_views(win))
    return ps, arena, flats


@pytest.mark.parametrize("opt_name", ["Adam", "AdamW", "SGD", "SGD_wd0", "LARS"])
def test_optimizers_on_parameters_that_are_views_of_one_arena(opt_name):
    from mfvit import optim
    from moco.optimizer import LARS
    from oracle import ref_optim
    ps, arena, flats = _arena_setup(opt_name)
    kw = dict(Adam=dict(lr=1e-2, weight_decay=0.1), AdamW=dict(lr=1e-2, weight_decay=0.1), SGD=dict(lr=0.1, momentum=0.9, weight_decay=0.01),
              SGD_wd0=dict(lr=0.1, momentum=0.9, weight_decay=0.0), LARS=dict(lr=0.3, weight_decay=2.0 ** -6, momentum=0.9))[opt_name]
    cls = dict(Adam=optim.Adam, AdamW=optim.AdamW, SGD=optim.SGD, SGD_wd0=optim.SGD, LARS=LARS)[opt_name]
    opt = cls(ps, **kw)
    # The C ABI takes its hyperparameters as floats, so the step that runs is the one with the ROUNDED values, and that is what the float64
    # reference restates.  It matters for one quantity: 1 - float32(0.999) is 1.3e-5 (relative) below 0.001, and so is every gradient's share in
    # exp_avg_sq next to a run with beta2 = 0.999 in double - the bias correction uses the same rounded beta2, so the update itself does not see it.
    kw = {k: f32(v) for k, v in kw.items()}
    betas, eps, trust = (f32(0.9), f32(0.999)), f32(1e-8), f32(0.001)
    names = cls.state_names
    for i, p in enumerate(ps):
        if i != FROZEN:
            p.grad = flats["grad"][2][i]
            for k, nm in enumerate(names):
                opt.state[p][nm] = flats[f"s{k}"][2][i]
    if opt_name == "LARS":
        with torch.no_grad():
            ps[4].zero_()                                              # a zero 2-D parameter: q = 1
    rtol, atol = (LARS_RTOL, LARS_ATOL) if opt_name == "LARS" else (ADAM_RTOL, ADAM_ATOL)
    worst = 0.0
    for s in range(3):
        if opt_name == "LARS" and s == 1:
            flats["grad"][2][7].copy_(-kw["weight_decay"] * ps[7].detach())     # zero update norm: q = 1
        before = dict(p=arena.flat.clone(), **{k: v[0].clone() for k, v in flats.items()})
        b_views = dict(p=arena.grad_views(before["p"]), **{k: arena.grad_views(before[k][PAD + ph:PAD + ph + arena.flat.numel()])
                                                            for k, ph in (("grad", 2), ("s0", 1), ("s1", 3))})
        opt.step()
        torch.cuda.synchronize()
        assert arena.intact()
        for k in ("grad", "s0", "s1"):       # gradients are read-only; states change only inside their window (s1: only Adam has one)
            keep = torch.zeros_like(flats[k][0], dtype=torch.bool)
            if k == "s0" or (k == "s1" and len(names) > 1):
                ph = dict(s0=1, s1=3)[k]
                keep[PAD + ph:PAD + ph + arena.flat.numel()] = True
            assert same_bits(flats[k][0], before[k], keep), (s, k)
        for i, p in enumerate(ps):
            if i == FROZEN:
                assert same_bits(p.detach(), b_views["p"][i]) and all(same_bits(flats[f"s{k}"][2][i], b_views[f"s{k}"][i]) for k in range(2))
                continue
            bp, bg, b0, b1 = (b_views[k][i] for k in ("p", "grad", "s0", "s1"))
            if opt_name.startswith("Adam"):
                ref = ref_optim.adam_step(bp, bg, b0, b1, s + 1, kw["lr"], betas[0], betas[1], eps, kw["weight_decay"], decoupled=opt_name == "AdamW")
                got = (p.detach(), flats["s0"][2][i], flats["s1"][2][i])
                assert int(opt.state[p]["step"]) == s + 1
            elif opt_name.startswith("SGD"):
                ref = ref_optim.sgd_step(bp, bg, b0, kw["lr"], kw["momentum"], kw["weight_decay"], first_step=False)      # a zero buffer IS the first step
                got = (p.detach(), flats["s0"][2][i])
            else:
                ref = ref_optim.lars_step(bp, bg, b0, kw["lr"], kw["weight_decay"], kw["momentum"], trust)
                got = (p.detach(), flats["s0"][2][i])
            for g_, r_ in zip(got, ref):
                e = ref_optim.gate_ratio(g_, r_, rtol, atol)
                worst = max(worst, e)
                assert e <= 1.0, (opt_name, s, i, e)
        flats["grad"][1].mul_(-0.7)
    log(f"{opt_name} on one arena[{len(ARENA_SHAPES)} parameters at phases 0..3, gradients / states at other phases, 3 steps] {worst:.2f} of the gate rtol {rtol:.0e} atol {atol:.0e}")
