"""Gradient-norm clipping on the optimizer chunk tables (csrc/optim.hip: grad_norm_kernel, grad_clip_coef_kernel, grad_scale_kernel;
mfvit.optim.clip_grad_norm_ / grad_norm) against the float64 restatement of torch.nn.utils.clip_grad_norm_ in tests/grad_clip_ref.py
(pinned to torch by tests/test_grad_clip_cpu.py, which also shows that the gate catches a dropped head, tail or second group).
(a) Raw tables over gradient views in NaN-padded flat buffers: every size edge of the head / 16-byte group / tail split at every phase, a
tensor over four table rows, rows in tensor order and interleaved - a single float read past a view puts a NaN into the total.
(b) Through mfvit.optim on parameters that are consecutive views of one arena, two param groups, one parameter without a gradient, with the
data-parallel hook and with mfvit.amp.GradScaler.
Gates (derived in grad_clip_ref.py, D = 44 roundings): norms (D / 2 + 1) u = 1.37e-6, scaled gradients (D / 2 + 3) u = 1.49e-6, relative,
atol 0; the inf norm is exact.  Measured errors are appended to parity_moco_ops.txt as multiples of the gate."""
import functools
import math

import pytest
import torch

import grad_clip_ref as ref
from test_optim_kernels_gpu import ADAM_ATOL, ADAM_RTOL, CHUNK_ROW, DEV, NAN, PAD, Flat, build_table, chunks_in_order, log, same_bits

pytestmark = pytest.mark.gpu
INF = float("inf")
KINDS = {2.0: 0, INF: 1}
norm_types = pytest.mark.parametrize("norm_type", [2.0, INF], ids=["l2", "inf"])


@functools.lru_cache(maxsize=None)
def setup():
    """(counts, float32 inputs, {norm_type: (per-tensor norms, total)}): computed once, never written."""
    from oracle import ref_optim
    assert ref.CHUNK == CHUNK_ROW
    counts = list(ref_optim.ADAM_COUNTS) + [3 * CHUNK_ROW + 5]
    vals = ref.inputs(counts)
    return counts, vals, {nt: ref.norm_ref(vals, nt) for nt in KINDS}


def orders(counts):
    """Table rows in tensor order, and with the four rows of the last tensor out of order among the others'."""
    rows = chunks_in_order(counts)
    small, big = rows[:-4], rows[-4:]
    assert all(t == len(counts) - 1 for t, _ in big)
    mixed = [big[2]] + small[:9] + [big[0]] + small[9:18] + [big[3]] + small[18:][::-1] + [big[1]]
    assert sorted(mixed) == rows
    return {"in_order": rows, "interleaved": mixed}


def phases(n, shift):
    return [(shift + i) % 4 for i in range(n)]


def run(tables, nts, norm_type, max_norm=INF, scale=False):
    """The three entry points over one or more tables as one call of mfvit.optim does: (out2, per-tensor norms), scratch between NaN guard bands."""
    from mfvit._lib import check, lib, ptr, stream
    kind = KINDS[norm_type]
    nrows, nt = sum(t.shape[0] for t in tables), sum(nts)
    pbuf = torch.full((PAD + nrows + PAD,), NAN, device=DEV)
    obuf = torch.full((PAD + 2 + PAD,), NAN, device=DEV)
    nbuf = torch.full((PAD + nt + PAD,), NAN, device=DEV)
    part, out, norms = pbuf[PAD:PAD + nrows], obuf[PAD:PAD + 2], nbuf[PAD:PAD + nt]
    row, base, rts = 0, 0, []
    for t, n in zip(tables, nts):
        check(lib().mfvit_grad_norm_partials(ptr(t), t.shape[0], kind, part.data_ptr() + 4 * row, stream()), "mfvit_grad_norm_partials")
        rts.append(t[:, 0].to(torch.int32) + base)
        row += t.shape[0]
        base += n
    rt = torch.cat(rts)
    check(lib().mfvit_grad_clip_coef(ptr(part), ptr(rt), nrows, nt, kind, float(max_norm), ptr(norms), ptr(out), stream()), "mfvit_grad_clip_coef")
    if scale:
        for t in tables:
            check(lib().mfvit_grad_scale(ptr(t), t.shape[0], out.data_ptr() + 4, stream()), "mfvit_grad_scale")
    torch.cuda.synchronize()
    for buf, n in ((pbuf, nrows), (obuf, 2), (nbuf, nt)):
        assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all())
    return out.clone(), norms.clone()


def one_table(vals, counts, shift, order):
    G = Flat(counts, phases(len(counts), shift), vals)
    return G, build_table(order, counts, [G, G, None, None], [0] * len(counts))


def check_norms(out, norms, want, norm_type):
    """Gate ratios of (per-tensor norms, total); the inf norm must be exact."""
    per, total = want
    if norm_type == INF:
        assert torch.equal(norms.double().cpu(), per.cpu()) and float(out[0]) == float(total)
        return 0.0, 0.0
    return ref.rel_ratio(norms, per, ref.NORM_RTOL), ref.rel_ratio(out[0], total, ref.NORM_RTOL)


# ------------------------------------------------------------------------------------------------ raw tables
@norm_types
@pytest.mark.parametrize("order", ["in_order", "interleaved"])
def test_norm_pass_size_edges_phases_and_row_orders(order, norm_type):
    counts, vals, want = setup()
    worst = [0.0, 0.0]
    for shift in range(4):
        G, table = one_table(vals, counts, shift, orders(counts)[order])
        assert {(a // 4) % 4 for a in table[:, 2].tolist()} == {0, 1, 2, 3}
        before = G.buf.clone()
        out, norms = run([table], [len(counts)], norm_type)
        assert same_bits(G.buf, before)                                        # the gradients are read only
        e = check_norms(out, norms, want[norm_type], norm_type)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert max(e) <= 1.0, (shift, e)
        assert float(out[1]) == 1.0                                            # max_norm = inf: nothing to clip
    log(f"grad_norm_kernel[{norm_type}, {len(counts)} tensors in {len(orders(counts)[order])} rows {order}, 4 phase patterns] per-tensor {worst[0]:.2f} "
        f"total {worst[1]:.2f} of the gate rtol {ref.NORM_RTOL:.2e}")


@norm_types
def test_scale_pass_clips_inside_the_views_only(norm_type):
    counts, vals, want = setup()
    total = float(want[norm_type][1])
    worst = [0.0, 0.0]
    for shift in range(4):
        G, table = one_table(vals, counts, shift, orders(counts)["interleaved"])
        before = G.buf.clone()
        max_norm = 0.5 * total
        out, _ = run([table], [len(counts)], norm_type, max_norm, scale=True)
        _, coef, _, clipped = ref.clip_ref(vals, max_norm, norm_type)
        assert same_bits(G.buf, before, G.mask)                                # the NaNs between and around the views
        e_g = ref.rel_ratio(G.buf[G.mask], torch.cat(clipped), ref.GRAD_RTOL)
        new = ref.norm_ref([G.view(i) for i in range(len(counts))], norm_type)[1]
        e_n = ref.rel_ratio(new, torch.tensor(max_norm), ref.GRAD_RTOL)
        e_c = ref.rel_ratio(out[1], coef, ref.GRAD_RTOL)
        worst = [max(worst[0], e_g), max(worst[1], e_n)]
        assert max(e_g, e_n, e_c) <= 1.0, (shift, e_g, e_n, e_c)
        # under the bound: the coefficient is exactly 1 and no gradient bit moves
        G.buf.copy_(before)
        out, _ = run([table], [len(counts)], norm_type, 2.0 * total, scale=True)
        assert float(out[1]) == 1.0 and same_bits(G.buf, before)
    log(f"grad_scale_kernel[{norm_type}, max_norm = total / 2, 4 phase patterns] gradients {worst[0]:.2f} new norm {worst[1]:.2f} of the gate rtol {ref.GRAD_RTOL:.2e}")


@norm_types
def test_edges_zero_inf_and_nan(norm_type):
    counts, vals, _ = setup()
    order = orders(counts)["in_order"]
    # all-zero gradients: total 0, coefficient 1, nothing written
    zeros = [torch.zeros_like(v) for v in vals]
    G, table = one_table(zeros, counts, 1, order)
    before = G.buf.clone()
    out, norms = run([table], [len(counts)], norm_type, 1.0, scale=True)
    assert out.tolist() == [0.0, 1.0] and not bool(norms.any()) and same_bits(G.buf, before)
    # one inf: total inf, coefficient 0; finite elements become 0, the inf becomes NaN
    bad = [v.clone() for v in vals]
    bad[20][1000] = -INF
    G, table = one_table(bad, counts, 2, order)
    before = G.buf.clone()
    out, _ = run([table], [len(counts)], norm_type, 1.0, scale=True)
    total, coef, _, clipped = ref.clip_ref(bad, 1.0, norm_type)
    assert float(total) == INF and float(coef) == 0.0 and out.tolist() == [INF, 0.0]
    got, want = G.buf[G.mask].double().cpu(), torch.cat(clipped)
    assert int(torch.isnan(want).sum()) == 1 and torch.equal(torch.isnan(got), torch.isnan(want)) and not bool(got[~torch.isnan(got)].any())
    assert same_bits(G.buf, before, G.mask)
    # one NaN as the last tail element of the last tensor: a NaN total for either norm (fmaxf would drop it), every gradient becomes NaN
    bad = [v.clone() for v in vals]
    bad[-1][-1] = NAN
    for shift in range(4):
        G, table = one_table(bad, counts, shift, order)
        before = G.buf.clone()
        out, norms = run([table], [len(counts)], norm_type, 1.0, scale=True)
        assert math.isnan(float(out[0])) and math.isnan(float(out[1])), (shift, out)
        assert torch.isnan(norms).tolist() == [False] * (len(counts) - 1) + [True]
        assert bool(torch.isnan(G.buf).all()) and same_bits(G.buf, before, G.mask)


@norm_types
def test_two_tables_give_one_total(norm_type):
    """Two param groups: even and odd tensors in tables of their own (tensor ids local to each), partials side by side, one finalize."""
    counts, vals, _ = setup()
    idx = [list(range(0, len(counts), 2)), list(range(1, len(counts), 2))]
    cs = [[counts[i] for i in ix] for ix in idx]
    vs = [[vals[i] for i in ix] for ix in idx]
    Gs, tables = zip(*[one_table(v, c, s, chunks_in_order(c)[::-1]) for v, c, s in zip(vs, cs, (1, 3))])
    union = vs[0] + vs[1]
    out, norms = run(list(tables), [len(c) for c in cs], norm_type)
    e = check_norms(out, norms, ref.norm_ref(union, norm_type), norm_type)
    assert max(e) <= 1.0, e
    max_norm = 0.3 * float(out[0])
    out, _ = run(list(tables), [len(c) for c in cs], norm_type, max_norm, scale=True)
    clipped = ref.clip_ref(union, max_norm, norm_type)[3]
    e_g = ref.rel_ratio(torch.cat([G.buf[G.mask] for G in Gs]), torch.cat(clipped), ref.GRAD_RTOL)
    assert e_g <= 1.0, e_g
    log(f"grad clip[{norm_type}, two tables in one call] norms {max(e):.2f} of rtol {ref.NORM_RTOL:.2e}, gradients {e_g:.2f} of rtol {ref.GRAD_RTOL:.2e}")


@norm_types
def test_same_inputs_give_the_same_bits(norm_type):
    counts, vals, want = setup()
    res = []
    for _ in range(2):
        G, table = one_table(vals, counts, 3, orders(counts)["interleaved"])
        out, norms = run([table], [len(counts)], norm_type, 0.5 * float(want[norm_type][1]), scale=True)
        res.append((out, norms, G.buf[G.mask].clone()))
    assert all(same_bits(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ through mfvit.optim
SHAPES = [(3,), (5,), (1153,), (33, 7), (129, 3), (70000,), (3,), (257, 4), (6,)]      # a 3-element bias first: everything behind it is off a boundary
FROZEN = 3                                                                               # never gets a gradient
SPLIT = 5                                                                                # param groups: [0, 5) and [5, 9)
HYPER = dict(lr=1e-2, weight_decay=0.1)


def arena_setup():
    """Parameters as consecutive views of one arena, gradients as consecutive views of a NaN-guarded flat buffer two floats behind a boundary."""
    from conftest import rng_tensor
    from mfvit import optim
    from mfvit.arena import ParamArena
    ps = [torch.nn.Parameter(rng_tensor(7800 + i, s).to(DEV)) for i, s in enumerate(SHAPES)]
    arena = ParamArena([(f"p{i}", p) for i, p in enumerate(ps)])
    assert arena.intact() and {(p.data_ptr() // 4) % 4 for p in ps} == {0, 1, 2, 3}
    total = arena.flat.numel()
    gbuf = torch.full((PAD + 2 + total + PAD,), NAN, device=DEV)
    win = gbuf[PAD + 2:PAD + 2 + total]
    win.copy_(ref.boosted(rng_tensor(7900, (total,))).to(DEV))
    views = arena.grad_views(win)
    true = [v.clone() for v in views]
    opt = optim.Adam([dict(params=ps[:SPLIT]), dict(params=ps[SPLIT:])], **HYPER)
    live = [i for i in range(len(ps)) if i != FROZEN]
    return ps, arena, gbuf, views, true, opt, live


def adam_ref(p0, grads, live):
    from oracle import ref_optim
    from test_optim_kernels_gpu import f32
    return [ref_optim.adam_step(p0[i], g, torch.zeros_like(p0[i]), torch.zeros_like(p0[i]), 1, f32(HYPER["lr"]), f32(0.9), f32(0.999), f32(1e-8),
                                f32(HYPER["weight_decay"]))[0] for i, g in zip(live, grads)]


@norm_types
def test_clip_through_the_optimizer_on_one_arena(norm_type):
    from mfvit import optim
    ps, arena, gbuf, views, true, opt, live = arena_setup()
    # the data-parallel hook: the gradients of a group arrive (here: are written) when before_group(gi) joins its exchange - until then they are NaN
    calls, pending = [], {0: range(0, SPLIT), 1: range(SPLIT, len(ps))}
    for i in live:
        views[i].fill_(NAN)
        ps[i].grad = views[i]

    def before_group(gi):
        calls.append(gi)
        for i in pending.pop(gi, ()):
            views[i].copy_(true[i])
    opt.before_group = before_group
    p0 = [p.detach().clone() for p in ps]
    want_per, want_total = ref.norm_ref([true[i] for i in live], norm_type)
    max_norm = 0.5 * float(want_total)
    total, norms = optim.clip_grad_norm_(opt, max_norm, norm_type=norm_type, per_tensor=True)
    torch.cuda.synchronize()
    assert calls == [0, 1] and total.shape == () and total.dtype == torch.float32 and norms.shape == (len(live),)
    e = check_norms(torch.stack([total, total]), norms, (want_per, want_total), norm_type)
    clipped = ref.clip_ref([true[i] for i in live], max_norm, norm_type)[3]
    e_g = max(ref.rel_ratio(views[i], c, ref.GRAD_RTOL) for i, c in zip(live, clipped))
    assert max(e) <= 1.0 and e_g <= 1.0, (e, e_g)
    keep = torch.zeros_like(gbuf, dtype=torch.bool)
    keep[PAD + 2:PAD + 2 + arena.flat.numel()] = True
    assert bool(torch.isnan(gbuf[~keep]).all()) and same_bits(views[FROZEN], true[FROZEN])       # guard bands; the parameter without a gradient
    # a second call with unchanged addresses: the cached tables, no upload; grad_norm leaves the gradients alone and sees the clipped norm
    tabs = [(opt._cache()[gi]["last"][3][0], dict(opt._cache()[gi]["tables"])) for gi in range(2)]
    part = opt._cache()["clip"]["partials"]
    g_before = gbuf.clone()
    again = optim.grad_norm(opt, norm_type=norm_type)
    torch.cuda.synchronize()
    for gi, (t, d) in enumerate(tabs):
        c = opt._cache()[gi]
        assert c["last"][3][0] is t and len(c["tables"]) == 1 and all(c["tables"][k] is v for k, v in d.items())
    assert opt._cache()["clip"]["partials"] is part and same_bits(gbuf, g_before)
    assert ref.rel_ratio(again, torch.tensor(max_norm), ref.GRAD_RTOL) <= 1.0
    assert float(opt.clip_grad_norm_(4.0 * max_norm, norm_type=norm_type)) == float(again) and same_bits(gbuf, g_before)     # the method; under the bound
    # the step that follows runs on the clipped gradients
    opt.step()
    torch.cuda.synchronize()
    from oracle import ref_optim
    e_p = max(ref_optim.gate_ratio(ps[i].detach(), r, ADAM_RTOL, ADAM_ATOL) for i, r in zip(live, adam_ref(p0, clipped, live)))
    assert e_p <= 1.0 and arena.intact() and same_bits(ps[FROZEN].detach(), p0[FROZEN]), e_p
    assert calls == [0, 1] * 4
    log(f"clip_grad_norm_[{norm_type}, Adam, two param groups on one arena] norms {max(e):.2f} of rtol {ref.NORM_RTOL:.2e}, gradients {e_g:.2f} of rtol "
        f"{ref.GRAD_RTOL:.2e}, parameters after step() {e_p:.2f} of the gate rtol {ADAM_RTOL:.0e} atol {ADAM_ATOL:.0e}")


def scaler_backward(ps, true, live, scaler):
    """scaler.scale(loss).backward() of loss = sum <p, w>: every gradient is w * scale, exactly (the scale is a power of two)."""
    loss = sum((ps[i] * true[i]).sum() for i in live)
    scaler.scale(loss).backward()


def test_grad_scaler_flow_clips_between_unscale_and_step():
    from mfvit import optim
    from mfvit.amp import GradScaler
    from oracle import ref_optim
    ps, arena, _, _, true, opt, live = arena_setup()
    scaler = GradScaler(init_scale=2.0 ** 16)
    p0 = [p.detach().clone() for p in ps]
    max_norm = 0.5 * float(ref.norm_ref([true[i] for i in live])[1])
    scaler_backward(ps, true, live, scaler)
    assert all(torch.equal(ps[i].grad, true[i] * 65536.0) for i in live) and ps[FROZEN].grad is None
    scaler.unscale_(opt)
    total = optim.clip_grad_norm_(opt, max_norm)
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    clipped = ref.clip_ref([true[i] for i in live], max_norm)[3]
    assert ref.rel_ratio(total, ref.norm_ref([true[i] for i in live])[1], ref.NORM_RTOL) <= 1.0
    e_p = max(ref_optim.gate_ratio(ps[i].detach(), r, ADAM_RTOL, ADAM_ATOL) for i, r in zip(live, adam_ref(p0, clipped, live)))
    assert e_p <= 1.0 and scaler.get_scale() == 2.0 ** 16, e_p
    # an overflowed gradient: the total is inf, the step is skipped, the parameters keep their bits and the scale backs off
    p1 = arena.flat.clone()
    opt.zero_grad(set_to_none=True)
    scaler_backward(ps, true, live, scaler)
    ps[5].grad[4321] = INF
    scaler.unscale_(opt)
    total = optim.clip_grad_norm_(opt, max_norm)
    assert scaler.step(opt) is None
    scaler.update()
    torch.cuda.synchronize()
    assert float(total) == INF and same_bits(arena.flat, p1) and scaler.get_scale() == 2.0 ** 15
    assert all(int(opt.state[ps[i]]["step"]) == 1 for i in live)


def test_error_if_nonfinite_and_no_gradients():
    from mfvit import optim
    ps, _, _, views, true, opt, live = arena_setup()
    zero, norms = optim.clip_grad_norm_(opt, 1.0, per_tensor=True)             # no gradient anywhere: a zero, nothing to launch
    assert float(zero) == 0.0 and zero.is_cuda and norms.numel() == 0 and "partials" not in opt._cache().get("clip", {})
    for i in live:
        ps[i].grad = views[i]
    views[live[-1]][-1] = NAN
    before = [views[i].clone() for i in live]
    for norm_type in KINDS:
        with pytest.raises(RuntimeError, match="non-finite, so it cannot be clipped"):
            optim.clip_grad_norm_(opt, 1.0, norm_type=norm_type, error_if_nonfinite=True)
        assert all(same_bits(views[i], b) for i, b in zip(live, before))       # raised before the scale pass, as torch does
    other = optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)            # parameters on the CPU
    with pytest.raises(ValueError, match="one device"):
        optim.clip_grad_norm_([opt, other], 1.0)
    total = optim.clip_grad_norm_([opt], 1.0)                                  # a sequence of optimizers; NaN total -> every gradient NaN
    assert math.isnan(float(total)) and all(bool(torch.isnan(views[i]).all()) for i in live)
