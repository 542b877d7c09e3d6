"""SAM / ASAM on the optimizer chunk tables (csrc/optim.hip: sam_norm_adaptive_kernel, sam_scale_kernel, sam_perturb_kernel, sam_restore_kernel;
mfvit.optim.SAM) against the float64 restatement of tests/sam_ref.py (pinned to a plain-torch SAM by tests/test_sam_cpu.py, which also shows
that the gates catch a dropped head, tail or second group and that the element-wise restatement is sensitive to its mutations).
(a) Raw tables over views in NaN-padded flat buffers: every size edge of the head / 16-byte group / tail split with w, g and old_p sharing each
of the four phases and at mismatched phases, rows in order and interleaved; special values; two tables in one total; determinism.
(b) Through mfvit.optim.SAM on parameters that are views of one arena (over Adam and SGD, step(closure) against the two-call form), on a
vit_small whose split-bf16 weight shadows must follow the perturbed and the restored weights, and with mfvit.amp.GradScaler.
Gates (derived in sam_ref.py, D_A = 46 roundings): total norm and inv (D_A / 2 + 1) u = 1.43e-6 relative, atol 0; old_p, the perturbed and the
restored weights are compared for bits (the perturbed ones with a float32 restatement fed the device's own inv)."""
import functools
import math

import pytest
import torch

import grad_clip_ref as gref
import sam_ref as ref
from test_optim_kernels_gpu import ADAM_ATOL, ADAM_RTOL, CHUNK_ROW, DEV, NAN, PAD, Flat, build_table, chunks_in_order, f32, log, same_bits

pytestmark = pytest.mark.gpu
INF = float("inf")
RHO = f32(0.05)
# (w, g, old_p) phases of tensor 0 - tensor i is i floats further on in all three, so every tensor meets every phase and the relation holds.
SHARED = [(s, s, s) for s in range(4)]
MIXED = [(0, 1, 2), (1, 3, 0), (3, 2, 1),            # every pair differs
         (0, 0, 1), (2, 0, 2), (0, 3, 3),            # exactly one pair agrees: w = g, w = old_p, g = old_p
         (1, 1, 0), (2, 3, 0)]                       # old_p on a boundary (tensor 0) while w and g are off it
orders_ = pytest.mark.parametrize("order", ["in_order", "interleaved"])
adaptives_ = pytest.mark.parametrize("adaptive", [0, 1], ids=["sam", "asam"])


@functools.lru_cache(maxsize=None)
def setup():
    """(counts, w, g, {adaptive: (norm, inv, e, perturbed w)} for rho = RHO): computed once, never written."""
    assert ref.CHUNK == CHUNK_ROW
    counts = list(ref.COUNTS)
    ws, gs = ref.inputs(counts)
    n = len(counts)
    return counts, ws, gs, {a: ref.first_step_ref(ws, gs, [RHO] * n, [bool(a)] * n) for a in (0, 1)}


def orders(counts):
    rows = chunks_in_order(counts)
    mixed = rows[1::2][::-1] + rows[0::2]
    assert sorted(mixed) == rows and mixed != rows
    return {"in_order": rows, "interleaved": mixed}


def flats(counts, ws, gs, triple):
    """W, G, O (old_p: NaN everywhere, so an element the kernel did not write shows) at the phases of `triple`."""
    ph = [[(p + i) % 4 for i in range(len(counts))] for p in triple]
    nans = [torch.full((c,), NAN) for c in counts]
    return Flat(counts, ph[0], ws), Flat(counts, ph[1], gs), Flat(counts, ph[2], nans)


def guarded(n):
    buf = torch.full((PAD + n + PAD,), NAN, device=DEV)
    return buf, buf[PAD:PAD + n]


def guards_ok(buf, n):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all())


def first_pass(tables, adaptives, rhos, found=None, perturb=True):
    """The three entry points over one or more tables as SAM.first_step calls them: (out2 clone, partials clone, device out2)."""
    from mfvit._lib import check, lib, ptr, stream
    nrows = sum(t.shape[0] for t in tables)
    pbuf, part = guarded(nrows)
    obuf, out = guarded(2)
    row = 0
    for t, a in zip(tables, adaptives):
        check(lib().mfvit_sam_norm_partials(ptr(t), t.shape[0], int(a), part.data_ptr() + 4 * row, stream()), "mfvit_sam_norm_partials")
        row += t.shape[0]
    check(lib().mfvit_sam_scale(ptr(part), nrows, ptr(found), ptr(out), stream()), "mfvit_sam_scale")
    if perturb:
        for t, r in zip(tables, rhos):
            check(lib().mfvit_sam_perturb(ptr(t), t.shape[0], out.data_ptr() + 4, r, stream()), "mfvit_sam_perturb")
    torch.cuda.synchronize()
    assert guards_ok(pbuf, nrows) and guards_ok(obuf, 2)
    return out.clone(), part.clone(), out


def restore(tables, out):
    from mfvit._lib import check, lib, ptr, stream
    for t in tables:
        check(lib().mfvit_sam_restore(ptr(t), t.shape[0], out.data_ptr() + 4, stream()), "mfvit_sam_restore")
    torch.cuda.synchronize()


def restated(ws, gs, inv, rho, adaptive):
    return torch.cat([ref.perturb_f32(w, g, inv, rho, adaptive) for w, g in zip(ws, gs)])


# ------------------------------------------------------------------------------------------------ raw tables
@adaptives_
@orders_
def test_size_edges_shared_and_mismatched_phases_and_row_orders(order, adaptive):
    counts, ws, gs, want = setup()
    norm, inv, es, pert = want[adaptive]
    worst = [0.0, 0.0]
    for triple in SHARED + MIXED:
        W, G, O = flats(counts, ws, gs, triple)
        table = build_table(orders(counts)[order], counts, [W, G, O, None], [adaptive] * len(counts))
        if triple in SHARED:
            assert {a % 16 for a in table[:, 1].tolist()} == {0, 4, 8, 12} and all((r[1] ^ r[2]) % 16 == 0 == (r[1] ^ r[3]) % 16 for r in table.tolist())
        else:
            assert all((r[1] ^ r[2]) % 16 or (r[1] ^ r[3]) % 16 for r in table.tolist())
        w0, g0, o0 = W.buf.clone(), G.buf.clone(), O.buf.clone()
        out, _, dev_out = first_pass([table], [adaptive], [RHO])
        e_n, e_i = ref.rel_ratio(out[0], norm, ref.NORM_RTOL), ref.rel_ratio(out[1], inv, ref.INV_RTOL)
        worst = [max(worst[0], e_n), max(worst[1], e_i)]
        assert max(e_n, e_i) <= 1.0, (triple, e_n, e_i)
        assert same_bits(G.buf, g0)                                                        # the gradients are read only
        assert same_bits(O.buf[O.mask], w0[W.mask]) and same_bits(O.buf, o0, O.mask)       # old_p = the old w, inside the views only
        assert same_bits(W.buf, w0, W.mask)                                                # the NaNs between and around the views
        got = W.buf[W.mask].cpu()
        assert same_bits(got, restated(ws, gs, float(out[1]), RHO, adaptive)), triple
        assert not same_bits(got, w0[W.mask].cpu())
        assert ref.perturbed_ratio(got, torch.cat(pert), torch.cat(es)) <= 1.0
        restore([table], dev_out)
        assert same_bits(W.buf, w0) and same_bits(G.buf, g0), triple
    log(f"sam kernels[{'asam' if adaptive else 'sam'}, {len(counts)} tensors in {len(orders(counts)[order])} rows {order}, {len(SHARED)} shared + "
        f"{len(MIXED)} mismatched phase patterns] norm {worst[0]:.2f} inv {worst[1]:.2f} of the gate rtol {ref.NORM_RTOL:.2e}; old_p, w + e, restored w bit-exact")


def test_plain_partials_are_the_clipping_kernels_bits():
    from mfvit._lib import check, lib, ptr, stream
    counts, ws, gs, _ = setup()
    for triple in [(1, 0, 2), (0, 1, 0), (3, 2, 1), (2, 3, 3)]:
        W, G, O = flats(counts, ws, gs, triple)
        table = build_table(orders(counts)["interleaved"], counts, [W, G, O, None], [0] * len(counts))
        _, part, _ = first_pass([table], [0], [RHO], perturb=False)
        pbuf, clip = guarded(table.shape[0])
        check(lib().mfvit_grad_norm_partials(ptr(table), table.shape[0], 0, ptr(clip), stream()), "mfvit_grad_norm_partials")
        torch.cuda.synchronize()
        assert same_bits(part, clip) and guards_ok(pbuf, table.shape[0])
        # the adaptive partials do not depend on w's phase either: the split is taken from the gradient pointer
        _, a0, _ = first_pass([table], [1], [RHO], perturb=False)
        W2, _, _ = flats(counts, ws, gs, (triple[1], 0, 0))
        table2 = build_table(orders(counts)["interleaved"], counts, [W2, G, O, None], [1] * len(counts))
        _, a1, _ = first_pass([table2], [1], [RHO], perturb=False)
        assert same_bits(a0, a1) and not same_bits(a0, part)


@adaptives_
def test_special_values_zero_inf_nan_and_the_scalers_flag(adaptive):
    counts, ws, gs, _ = setup()
    order = orders(counts)["in_order"]
    n = len(counts)
    # all-zero gradients: the norm is 0, inv = 1e12 is finite, e = 0 and no parameter moves
    W, G, O = flats(counts, ws, [torch.zeros_like(g) for g in gs], (1, 1, 1))
    table = build_table(order, counts, [W, G, O, None], [adaptive] * n)
    w0 = W.buf.clone()
    out, _, dev_out = first_pass([table], [adaptive], [RHO])
    assert float(out[0]) == 0.0 and float(out[1]) == f32(1e12) and same_bits(W.buf, w0) and same_bits(O.buf[O.mask], w0[W.mask])
    restore([table], dev_out)
    assert same_bits(W.buf, w0)
    # an inf, a NaN (the last tail element of the last tensor), or the GradScaler's flag on clean gradients: inv == 0 exactly, nothing moves
    cases = []
    for name, where, val in (("inf", (10, 1000), -INF), ("nan", (n - 1, counts[-1] - 1), NAN), ("flag", None, None)):
        bad = [g.clone() for g in gs]
        if where:
            bad[where[0]][where[1]] = val
        cases.append((name, bad))
    for name, bad in cases:
        for triple in ((2, 2, 2), (0, 1, 3)):
            W, G, O = flats(counts, ws, bad, triple)
            table = build_table(order, counts, [W, G, O, None], [adaptive] * n)
            w0, g0, o0 = W.buf.clone(), G.buf.clone(), O.buf.clone()
            found = torch.full((1,), 1.0 if name == "flag" else 0.0, device=DEV)
            out, _, dev_out = first_pass([table], [adaptive], [RHO], found=found)
            tot = float(out[0])
            assert (tot == INF if name == "inf" else math.isnan(tot) if name == "nan" else 0.0 < tot < INF), (name, tot)
            assert float(out[1]) == 0.0 and not math.copysign(1.0, float(out[1])) < 0, (name, out)
            assert same_bits(W.buf, w0) and same_bits(O.buf, o0) and same_bits(G.buf, g0), name        # old_p keeps its poison: not one byte moved
            restore([table], dev_out)
            assert same_bits(W.buf, w0) and same_bits(O.buf, o0), name                                 # ... and none of the poison came back
            assert float(found) == (1.0 if name == "flag" else 0.0)                                    # the flag is read only
    # a flag of 0 behind a non-NULL pointer perturbs as usual
    W, G, O = flats(counts, ws, gs, (0, 0, 0))
    table = build_table(order, counts, [W, G, O, None], [adaptive] * n)
    w0 = W.buf.clone()
    out, _, _ = first_pass([table], [adaptive], [RHO], found=torch.zeros(1, device=DEV))
    assert float(out[1]) > 0.0 and not same_bits(W.buf, w0)


def test_two_tables_with_their_own_rho_give_one_total():
    """Two param groups: even tensors plain with rho 0.05, odd tensors adaptive with rho 0.3, partials side by side, one scale."""
    counts, ws, gs, _ = setup()
    idx = [list(range(0, len(counts), 2)), list(range(1, len(counts), 2))]
    rhos, ads = [f32(0.05), f32(0.3)], [0, 1]
    sub = [([counts[i] for i in ix], [ws[i] for i in ix], [gs[i] for i in ix]) for ix in idx]
    Fs = [flats(c, w, g, t) for (c, w, g), t in zip(sub, ((1, 1, 1), (3, 0, 3)))]
    tables = [build_table(chunks_in_order(c)[::-1], c, [W, G, O, None], [a] * len(c)) for (c, _, _), (W, G, O), a in zip(sub, Fs, ads)]
    w0 = [F[0].buf.clone() for F in Fs]
    u_w, u_g = sub[0][1] + sub[1][1], sub[0][2] + sub[1][2]
    u_r = [rhos[0]] * len(idx[0]) + [rhos[1]] * len(idx[1])
    u_a = [False] * len(idx[0]) + [True] * len(idx[1])
    norm, inv, es, pert = ref.first_step_ref(u_w, u_g, u_r, u_a)
    out, _, dev_out = first_pass(tables, ads, rhos)
    e_n, e_i = ref.rel_ratio(out[0], norm, ref.NORM_RTOL), ref.rel_ratio(out[1], inv, ref.INV_RTOL)
    assert max(e_n, e_i) <= 1.0, (e_n, e_i)
    for (c, w, g), (W, G, O), r, a, b in zip(sub, Fs, rhos, ads, w0):
        assert same_bits(W.buf[W.mask].cpu(), restated(w, g, float(out[1]), r, a)) and same_bits(O.buf[O.mask], b[W.mask])
    got = torch.cat([F[0].buf[F[0].mask] for F in Fs])
    assert ref.perturbed_ratio(got, torch.cat(pert), torch.cat(es)) <= 1.0
    restore(tables, dev_out)
    assert all(same_bits(F[0].buf, b) for F, b in zip(Fs, w0))
    log(f"sam kernels[two tables, plain rho 0.05 + adaptive rho 0.3, one total] norm {e_n:.2f} inv {e_i:.2f} of the gate rtol {ref.NORM_RTOL:.2e}")


@adaptives_
def test_same_inputs_give_the_same_bits(adaptive):
    counts, ws, gs, _ = setup()
    res = []
    for _ in range(2):
        W, G, O = flats(counts, ws, gs, (3, 3, 3))
        table = build_table(orders(counts)["interleaved"], counts, [W, G, O, None], [adaptive] * len(counts))
        out, part, _ = first_pass([table], [adaptive], [RHO])
        res.append((out, part, W.buf[W.mask].clone(), O.buf[O.mask].clone()))
    assert all(same_bits(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ through mfvit.optim.SAM
SHAPES = [(3,), (5,), (1153,), (33, 7), (129, 3), (70000,), (3,), (257, 4), (6,)]      # a 3-element bias first: everything behind it is off a boundary
FROZEN = 3                                                                               # never gets a gradient
SPLIT = 5                                                                                # param groups: [0, 5) plain rho 0.05, [5, 9) adaptive rho 0.3
GROUPS = [dict(rho=0.05, adaptive=False), dict(rho=0.3, adaptive=True)]
BASES = {"Adam": dict(lr=1e-2, weight_decay=0.1), "SGD": dict(lr=0.1, momentum=0.9, weight_decay=0.01)}


def arena_setup(base, **kw):
    """Parameters as consecutive views of one arena, gradients as consecutive views of a NaN-guarded flat buffer two floats behind a boundary
    (w and g never share a phase, old_p comes from the allocator: the element-by-element path; the encoder test below takes the 16-byte one)."""
    from conftest import rng_tensor
    from mfvit import optim
    from mfvit.arena import ParamArena
    ps = [torch.nn.Parameter(rng_tensor(8900 + i, s).to(DEV)) for i, s in enumerate(SHAPES)]
    arena = ParamArena([(f"p{i}", p) for i, p in enumerate(ps)])
    assert arena.intact() and {(p.data_ptr() // 4) % 4 for p in ps} == {0, 1, 2, 3}
    total = arena.flat.numel()
    gbuf = torch.full((PAD + 2 + total + PAD,), NAN, device=DEV)
    win = gbuf[PAD + 2:PAD + 2 + total]
    win.zero_()
    views = arena.grad_views(win)
    true = arena.grad_views(ref.boosted(rng_tensor(8950, (total,))).to(DEV))
    sam = optim.SAM([dict(params=ps[:SPLIT], **GROUPS[0]), dict(params=ps[SPLIT:], **GROUPS[1])], getattr(optim, base), **dict(BASES[base], **kw))
    live = [i for i in range(len(ps)) if i != FROZEN]
    return ps, arena, gbuf, views, true, sam, live


def backward(ps, views, true, live, scale=1.0):
    """The gradient of sum_i 0.5 (i + 1) |p_i|^2 + <p_i, true_i>, times `scale` (a power of two: exact), written into the gradient views."""
    for i in live:
        views[i].copy_(((i + 1) * ps[i].detach() + true[i]) * scale)
        ps[i].grad = views[i]


def base_ref(base, p0, g, kw):
    from oracle import ref_optim
    if base == "Adam":
        return ref_optim.adam_step(p0, g, torch.zeros_like(p0), torch.zeros_like(p0), 1, f32(kw["lr"]), f32(0.9), f32(0.999), f32(1e-8), f32(kw["weight_decay"]))[0]
    return ref_optim.sgd_step(p0, g, torch.zeros_like(p0), f32(kw["lr"]), f32(kw["momentum"]), f32(kw["weight_decay"]), first_step=False)[0]


@pytest.mark.parametrize("base", ["Adam", "SGD"])
def test_one_sam_step_through_the_wrapper_on_one_arena(base):
    from oracle import ref_optim
    ps, arena, gbuf, views, true, sam, live = arena_setup(base)
    calls = []
    sam.before_group = calls.append
    p0 = [p.detach().clone() for p in ps]
    backward(ps, views, true, live)
    g1 = [views[i].clone() for i in live]
    rhos = [f32(GROUPS[i >= SPLIT]["rho"]) for i in live]
    ads = [GROUPS[i >= SPLIT]["adaptive"] for i in live]
    norm, inv, es, pert = ref.first_step_ref([p0[i] for i in live], g1, rhos, ads)
    sam.first_step()
    torch.cuda.synchronize()
    out = sam._pending[1]
    e_n, e_i = ref.rel_ratio(out[0], norm, ref.NORM_RTOL), ref.rel_ratio(out[1], inv, ref.INV_RTOL)
    assert max(e_n, e_i) <= 1.0 and calls == [0, 1], (e_n, e_i, calls)
    for k, i in enumerate(live):
        want = ref.perturb_f32(p0[i].cpu().flatten(), g1[k].cpu().flatten(), float(out[1]), rhos[k], ads[k])
        assert same_bits(ps[i].detach().cpu().flatten(), want), i
        assert same_bits(sam.state[ps[i]]["old_p"], p0[i]) and ref.perturbed_ratio(ps[i].detach(), pert[k], es[k]) <= 1.0
        assert same_bits(views[i], g1[k])
    assert same_bits(ps[FROZEN].detach(), p0[FROZEN]) and ps[FROZEN] not in sam.state and arena.intact()
    with pytest.raises(RuntimeError, match="twice"):
        sam.first_step()
    # the second backward at w + e; the base step starts from the restored bits and runs on these gradients
    backward(ps, views, true, live)
    g2 = [views[i].clone() for i in live]
    assert not any(same_bits(a, b) for a, b in zip(g1, g2))
    assert sam.second_step() is None
    torch.cuda.synchronize()
    e_p = max(ref_optim.gate_ratio(ps[i].detach(), base_ref(base, p0[i], g2[k], BASES[base]), ADAM_RTOL, ADAM_ATOL) for k, i in enumerate(live))
    assert e_p <= 1.0 and arena.intact() and same_bits(ps[FROZEN].detach(), p0[FROZEN]), e_p
    assert sam.base_optimizer.before_group == calls.append and calls[:4] == [0, 1, 0, 1] and sorted(set(calls)) == [0, 1]
    keep = torch.zeros_like(gbuf, dtype=torch.bool)
    keep[PAD + 2:PAD + 2 + arena.flat.numel()] = True
    assert bool(torch.isnan(gbuf[~keep]).all())
    with pytest.raises(RuntimeError, match="first_step"):
        sam.second_step()
    log(f"SAM[{base}, plain + adaptive param groups on one arena] norm {e_n:.2f} inv {e_i:.2f} of rtol {ref.NORM_RTOL:.2e}, parameters after "
        f"second_step() {e_p:.2f} of the gate rtol {ADAM_RTOL:.0e} atol {ADAM_ATOL:.0e}")


@pytest.mark.parametrize("base", ["Adam", "SGD"])
def test_step_with_a_closure_is_the_two_call_form(base):
    flat = []
    for form in ("closure", "two_calls"):
        ps, arena, _, views, true, sam, live = arena_setup(base)
        p0 = arena.flat.clone()
        seen = []

        def closure():
            assert torch.is_grad_enabled() and all(ps[i].grad is None for i in live)      # first_step(zero_grad=True) ran
            seen.append(arena.flat.clone())
            backward(ps, views, true, live)
        for _ in range(2):
            backward(ps, views, true, live)
            if form == "closure":
                sam.step(closure)
            else:
                sam.first_step(zero_grad=True)
                closure()
                sam.second_step()
        torch.cuda.synchronize()
        assert len(seen) == 2 and not same_bits(seen[0], p0) and not same_bits(arena.flat, p0) and arena.intact()
        flat.append((arena.flat.clone(), seen[0], seen[1]))
    assert all(same_bits(a, b) for a, b in zip(*flat))


def test_the_weight_shadows_follow_the_perturbed_and_the_restored_weights():
    from conftest import rng_tensor
    from mfvit import optim
    from test_encoder_gpu import build
    m, _ = build("bf16x3", 931, depth=2, img=32)
    x = rng_tensor(932, (4, 3, 32, 32)).to(DEV)
    sam = optim.SAM(m.parameters(), optim.Adam, rho=2.0, lr=0.0)
    first = m(x)
    first.square().sum().backward()
    live = [p for p in m.parameters() if p.grad is not None]
    before = [p.detach().clone() for p in live]
    sam.first_step(zero_grad=True)
    second = m(x)                                                  # must run on w + e: the shadows are rebuilt
    torch.cuda.synchronize()
    moved = sum(not same_bits(p.detach(), b) for p, b in zip(live, before))      # (a gradient that is zero throughout, the key bias', moves nothing)
    assert len(live) > 20 and moved > len(live) // 2, (moved, len(live))
    assert not torch.equal(second, first) and float((second - first).detach().abs().max()) > 1e-3 * float(first.detach().abs().max())
    twin, _ = build("bf16x3", 933, depth=2, img=32)
    twin.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert same_bits(twin(x), second.detach())
    second.square().sum().backward()
    sam.second_step(zero_grad=True)                                # lr = 0: the restored weights, bit for bit
    with torch.no_grad():
        third = m(x)
    torch.cuda.synchronize()
    assert all(same_bits(p.detach(), b) for p, b in zip(live, before)) and same_bits(third, first.detach())


def test_grad_scaler_flow_skips_on_an_overflow_in_either_pass():
    from mfvit.amp import GradScaler
    S = 2.0 ** 16

    def one_step(sam, scaler, ps, views, true, live, poison=None, clip=False):
        scale = scaler.get_scale() if scaler else 1.0
        backward(ps, views, true, live, scale)
        if poison == "first":
            views[5].view(-1)[4321] = INF
        sam.first_step(zero_grad=True, scaler=scaler)
        backward(ps, views, true, live, scale)
        if poison == "second":
            views[7].view(-1)[11] = NAN
        if clip:                                                   # torch's order: unscale, clip, step - second_step must not unscale again
            scaler.unscale_(sam.base_optimizer)
            total = sam.clip_grad_norm_(1e30)
            assert 0.0 < float(total) < 1e30
        ret = sam.second_step(zero_grad=True, scaler=scaler)
        if scaler:
            scaler.update()
        torch.cuda.synchronize()
        return ret

    # a clean scaled step is the unscaled step (the scale is a power of two)
    ps, arena, _, views, true, sam, live = arena_setup("Adam")
    one_step(sam, None, ps, views, true, live)
    plain = arena.flat.clone()
    ps, arena, _, views, true, sam, live = arena_setup("Adam")
    scaler = GradScaler(init_scale=S)
    p0 = arena.flat.clone()
    one_step(sam, scaler, ps, views, true, live)
    e = gref.rel_ratio(arena.flat, plain, gref.GRAD_RTOL)
    assert e <= 1.0 and not same_bits(arena.flat, p0) and scaler.get_scale() == S, e
    assert all(int(sam.base_optimizer.state[ps[i]]["step"]) == 1 for i in live)
    # an overflow in the first backward, then in the second: the weights end at their pre-step bits, the base state is untouched, the scale halves
    for k, poison in enumerate(("first", "second")):
        p1 = arena.flat.clone()
        st1 = {i: {n: t.clone() for n, t in sam.base_optimizer.state[ps[i]].items()} for i in live}
        assert one_step(sam, scaler, ps, views, true, live, poison) is None
        assert same_bits(arena.flat, p1) and scaler.get_scale() == S / 2 ** (k + 1), poison
        for i in live:
            assert all(same_bits(t.float(), st1[i][n].float()) for n, t in sam.base_optimizer.state[ps[i]].items()), (poison, i)
    # and the step after them runs again, here with a clip_grad_norm_ that does not clip between the second backward and second_step
    p2 = arena.flat.clone()
    one_step(sam, scaler, ps, views, true, live, clip=True)
    assert not same_bits(arena.flat, p2) and all(int(sam.base_optimizer.state[ps[i]]["step"]) == 2 for i in live)
    assert scaler.get_scale() == S / 4 and sam._pending is None
