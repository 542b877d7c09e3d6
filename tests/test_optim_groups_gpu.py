"""Group-aware optimizer steps (csrc/optim.hip: adam_groups_kernel, sgd_groups_kernel behind mfvit_adam_step_groups / mfvit_sgd_step_groups) and what
stands on them: mfvit.optim.{Adam, AdamW, SGD}(single_launch=True) with GradScaler and clipping on the joined table, param_groups_layer_decay on a
model, ModelEma.
(a) Raw entries over hand-built tables in NaN-padded buffers: BIT-equal to the per-group entry points (mfvit_adam_step / mfvit_sgd_step run once
per hyper entry over that entry's rows on cloned buffers) and inside the Adam gate of the float64 reference applied row by row
(tests/optim_groups_ref.py, pinned to torch.optim by tests/test_optim_groups_cpu.py, which also shows that the gate sees a wrong entry).
(b) Through the optimizers on parameters that are views of one arena, six groups: single_launch=True against False on twins, bit for bit, with
the launches counted at the ctypes boundary (host only)."""
import copy
import functools

import pytest
import torch

import optim_groups_ref as ref
from test_optim_kernels_gpu import ADAM_ATOL, ADAM_RTOL, CHUNK_ROW, DEV, FROZEN, Flat, _arena_setup, build_table, chunks_in_order, phases_for, \
    same_bits

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def raw_setup():
    """(counts, {p, g, m, v: float32 values per tensor}): computed once, never written."""
    from conftest import rng_tensor
    from oracle import ref_optim
    assert ref.CHUNK == CHUNK_ROW
    counts = list(ref_optim.ADAM_COUNTS) + [3 * CHUNK_ROW + 5]          # the last tensor: four table rows
    vals = {k: [rng_tensor(9000 + 10 * i + j, (c,), scale=s) for i, c in enumerate(counts)]
            for j, (k, s) in enumerate((("p", 1.0), ("g", 1.0), ("m", 0.1), ("v", 0.1)))}
    vals["v"] = [v.abs() for v in vals["v"]]
    return counts, vals


def set_flag_column(table, values):
    table[:, 6] = torch.tensor(values, dtype=torch.int64, device=DEV)


def per_tensor_of(buf, flat, counts):
    """Per-tensor CPU tensors of a buffer laid out like `flat`."""
    host = buf.cpu()
    return [host[o:o + c] for o, c in zip(flat.offs, counts)]


# ------------------------------------------------------------------------------------------------ 1. raw entry, Adam / AdamW
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_adam_groups_kernel_is_the_per_group_kernel_row_by_row(decoupled):
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_optim
    counts, vals = raw_setup()
    nt = len(counts)
    order = chunks_in_order(counts)
    rows = ref.rows_of(counts)
    assert [(t, a // CHUNK_ROW) for t, a, _ in rows] == order
    paths, worst = set(), {}
    for ai, align in enumerate(ref_optim.ADAM_ALIGN):
        for ci, nentries in enumerate(ref.ENTRY_COUNTS):
            entries = ref.adam_entries(nentries, decoupled)
            entry_of_row = ref.row_entries(len(rows), nentries, "interleaved" if (ai + ci) % 2 == 0 else "adjacent")
            assert entry_of_row[0] == nentries - 1 and (nentries == 1 or len(set(entry_of_row)) > 1)
            # F: the buffers of the group-aware launch; R: their clones for the per-group entry point
            F = {k: Flat(counts, phases_for(nt, align in (k, "all")), vals[k]) for k in "pgmv"}
            R = {k: Flat(counts, phases_for(nt, align in (k, "all")), vals[k]) for k in "pgmv"}
            table = build_table(order, counts, [F[k] for k in "pgmv"], [0] * nt)
            rtable = build_table(order, counts, [R[k] for k in "pgmv"], [0] * nt)
            # the joined table's flag column: the entry in the upper half; the lower half is not read (here: the opposite of the entry's bit)
            set_flag_column(table, [(k << 32) | int(not entries[k]["decoupled"]) for k in entry_of_row])
            set_flag_column(rtable, [int(entries[k]["decoupled"]) for k in entry_of_row])
            for row in table.tolist():
                aligned = all(a % 16 == 0 for a in row[1:5])
                assert aligned == (align == "aligned")
                paths |= {(aligned, int(x)) for x in set(ref_optim.adam_path_of(row[5], aligned).tolist())}
            rsel = [(k, torch.tensor([r for r, e in enumerate(entry_of_row) if e == k], device=DEV)) for k in sorted(set(entry_of_row))]
            rsub = [(k, rtable[idx].contiguous()) for k, idx in rsel]
            for s in range(3):
                before = {k: F[k].buf.clone() for k in "pgmv"}
                check(lib().mfvit_adam_step_groups(ptr(table), table.shape[0], ref.adam_hyper(entries, s), nentries, stream()), "mfvit_adam_step_groups")
                for k, sub in rsub:
                    e = entries[k]
                    check(lib().mfvit_adam_step(ptr(sub), sub.shape[0], e["lr"], e["beta1"], e["beta2"], e["eps"], e["weight_decay"], e["step"] + s,
                                                stream()), "mfvit_adam_step")
                torch.cuda.synchronize()
                assert same_bits(F["g"].buf, before["g"]) and same_bits(R["g"].buf, before["g"])
                for k in "pmv":
                    assert same_bits(F[k].buf, R[k].buf), (align, nentries, s, k)                     # the parent's path, bit for bit
                    assert same_bits(F[k].buf, before[k], F[k].mask), (align, nentries, s, k)         # the NaNs between and around the views
                    assert not same_bits(F[k].buf, before[k])
                want = ref.adam_rows_ref(rows, entry_of_row, entries, *[per_tensor_of(before[k], F[k], counts) for k in "pgmv"], step_offset=s)
                for k, w in zip("pmv", want):
                    e = ref_optim.gate_ratio(F[k].buf[F[k].mask], torch.cat(w), ADAM_RTOL, ADAM_ATOL)
                    worst[k] = max(worst.get(k, 0.0), e)
                    assert e <= 1.0, (align, nentries, s, k, e)
                for X in (F, R):
                    X["g"].buf.mul_(-0.7)                                                             # another gradient for the next step
    print(f"adam_groups_kernel[{'AdamW' if decoupled else 'Adam'}] worst gate ratios {worst}")
    assert paths == {(True, 0), (True, 1), (True, 2), (False, 3)}, paths


# ------------------------------------------------------------------------------------------------ 2. raw entry, SGD
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_groups_kernel_is_the_per_group_kernel_row_by_row(momentum):
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_optim
    counts, vals = raw_setup()
    nt = len(counts)
    order = chunks_in_order(counts)
    rows = ref.rows_of(counts)
    worst = 0.0
    for ai, align in enumerate(("aligned", "p", "g", "m", "all")):
        for ci, nentries in enumerate(ref.ENTRY_COUNTS):
            entries = ref.sgd_entries(nentries, momentum)
            entry_of_row = ref.row_entries(len(rows), nentries, "interleaved" if (ai + ci) % 2 == 0 else "adjacent")
            F = {k: Flat(counts, phases_for(nt, align in (k, "all")), vals[k]) for k in "pgm"}
            R = {k: Flat(counts, phases_for(nt, align in (k, "all")), vals[k]) for k in "pgm"}
            # momentum == 0: the kernel must not touch the state at all - its column of the table is a null pointer
            table = build_table(order, counts, [F["p"], F["g"], F["m"] if momentum else None, None], [0] * nt)
            rtable = build_table(order, counts, [R["p"], R["g"], R["m"] if momentum else None, None], [0] * nt)
            set_flag_column(table, [k << 32 for k in entry_of_row])
            rsub = [(k, rtable[torch.tensor([r for r, e in enumerate(entry_of_row) if e == k], device=DEV)].contiguous()) for k in sorted(set(entry_of_row))]
            for s in range(3):
                before = {k: F[k].buf.clone() for k in "pgm"}
                check(lib().mfvit_sgd_step_groups(ptr(table), table.shape[0], ref.sgd_hyper(entries), nentries, stream()), "mfvit_sgd_step_groups")
                for k, sub in rsub:
                    e = entries[k]
                    check(lib().mfvit_sgd_step(ptr(sub), sub.shape[0], e["lr"], e["momentum"], e["weight_decay"], 0, stream()), "mfvit_sgd_step")
                torch.cuda.synchronize()
                assert same_bits(F["g"].buf, before["g"])
                for k in "pm":
                    assert same_bits(F[k].buf, R[k].buf), (align, nentries, s, k)
                    assert same_bits(F[k].buf, before[k], F[k].mask), (align, nentries, s, k)
                assert not same_bits(F["p"].buf, before["p"]) and (bool(momentum) != same_bits(F["m"].buf, before["m"]))
                want = ref.sgd_rows_ref(rows, entry_of_row, entries, *[per_tensor_of(before[k], F[k], counts) for k in "pgm"])
                for k, w in zip("pm", want):
                    e = ref_optim.gate_ratio(F[k].buf[F[k].mask], torch.cat(w), ADAM_RTOL, ADAM_ATOL)
                    worst = max(worst, e)
                    assert e <= 1.0, (align, nentries, s, k, e)
                for X in (F, R):
                    X["g"].buf.mul_(-0.7)
    print(f"sgd_groups_kernel[momentum {momentum}] worst gate ratio {worst:.2f}")


# ------------------------------------------------------------------------------------------------ 3. argument errors
def test_bad_arguments_are_refused_and_an_entry_out_of_range_skips_its_row():
    from mfvit._lib import check, lib, ptr, stream
    counts = [1153, 7, 515, CHUNK_ROW + 3]                                                           # five rows: the last tensor has two
    from conftest import rng_tensor
    vals = {k: [rng_tensor(9400 + 10 * i + j, (c,)).abs() for i, c in enumerate(counts)] for j, k in enumerate("pgmv")}
    F = {k: Flat(counts, [0] * 4, vals[k]) for k in "pgmv"}
    R = {k: Flat(counts, [0] * 4, vals[k]) for k in "pgmv"}
    order = chunks_in_order(counts)
    table = build_table(order, counts, [F[k] for k in "pgmv"], [0] * 4)
    rtable = build_table(order, counts, [R[k] for k in "pgmv"], [1] * 4)
    entries = ref.adam_entries(2, True)
    hy = ref.adam_hyper(entries)
    h = lib()
    before = {k: F[k].buf.clone() for k in "pgmv"}
    assert h.mfvit_adam_step_groups(None, 5, hy, 2, stream()) == ref.EINVAL
    assert h.mfvit_adam_step_groups(ptr(table), 5, None, 2, stream()) == ref.EINVAL
    assert h.mfvit_adam_step_groups(ptr(table), 0, hy, 2, stream()) == ref.EINVAL
    assert h.mfvit_adam_step_groups(ptr(table), -1, hy, 2, stream()) == ref.EINVAL
    assert h.mfvit_adam_step_groups(ptr(table), 5, hy, 0, stream()) == ref.EINVAL
    bad = ref.adam_hyper(entries)
    bad[1].step = 0
    assert h.mfvit_adam_step_groups(ptr(table), 5, bad, 2, stream()) == ref.EINVAL
    sg = ref.sgd_hyper(ref.sgd_entries(2, 0.9))
    assert h.mfvit_sgd_step_groups(None, 5, sg, 2, stream()) == ref.EINVAL
    assert h.mfvit_sgd_step_groups(ptr(table), 5, None, 2, stream()) == ref.EINVAL
    assert h.mfvit_sgd_step_groups(ptr(table), 0, sg, 2, stream()) == ref.EINVAL
    assert h.mfvit_sgd_step_groups(ptr(table), 5, sg, 0, stream()) == ref.EINVAL
    torch.cuda.synchronize()
    assert all(same_bits(F[k].buf, before[k]) for k in "pgmv")                                      # refused: nothing ran
    # rows 0 and 2 (= tensors 0 and 2) name entries that do not exist (2: the first one past the end; 2^32 - 1: the largest index a row can hold)
    entry_of_row = [2, 0, 0xFFFFFFFF, 1, 1]
    assert order == [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1)]
    set_flag_column(table, [(k << 32) - (1 << 64 if k >> 31 else 0) for k in entry_of_row])         # (as a signed 64-bit value)
    for fn, tab, hyper in ((h.mfvit_adam_step_groups, table, hy), (h.mfvit_sgd_step_groups, None, sg)):
        if tab is None:      # SGD over the same buffers: p, g and the momentum buffer in m
            tab = table.clone()
            tab[:, 4] = 0
            rtable = rtable.clone()
            rtable[:, 4] = 0
        before = {k: F[k].buf.clone() for k in "pgmv"}
        for k in "pgmv":
            R[k].buf.copy_(before[k])
        check(fn(ptr(tab), 5, hyper, 2, stream()), "step_groups")
        for k in (0, 1):
            sub = rtable[torch.tensor([r for r, e in enumerate(entry_of_row) if e == k], device=DEV)].contiguous()
            e = entries[k]
            if fn is h.mfvit_adam_step_groups:
                check(h.mfvit_adam_step(ptr(sub), sub.shape[0], e["lr"], e["beta1"], e["beta2"], e["eps"], e["weight_decay"], e["step"], stream()), "adam")
            else:
                check(h.mfvit_sgd_step(ptr(sub), sub.shape[0], sg[k].lr, sg[k].momentum, sg[k].weight_decay, 0, stream()), "sgd")
        torch.cuda.synchronize()
        for k in "pgmv":
            assert same_bits(F[k].buf, R[k].buf), k                                                 # the other rows: the per-group path's bits
        for t in (0, 2):                                                                            # their rows were skipped: untouched
            for k in "pmv":
                o, c = F[k].offs[t], counts[t]
                assert same_bits(F[k].buf[o:o + c], before[k][o:o + c]), (t, k)
        assert not same_bits(F["p"].view(1), before["p"][F["p"].offs[1]:F["p"].offs[1] + counts[1]])
    assert entries[0]["decoupled"] and entries[1]["decoupled"]                                     # (rtable's flag 1 = what the entries say)


# ------------------------------------------------------------------------------------------------ the optimizers on one arena, six groups
class Calls:
    """Counts the calls of chosen C entry points at the ctypes boundary (host only) and records their order with the before_group calls."""

    def __init__(self, monkeypatch, names):
        from mfvit._lib import lib
        self.n, self.events, self.args = {k: 0 for k in names}, [], {}
        h = lib()
        for name in names:
            monkeypatch.setattr(h, name, self._wrap(name, getattr(h, name)), raising=True)

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            self.events.append(name)
            self.args[name] = a
            return fn(*a)
        return call

    def reset(self):
        self.n = {k: 0 for k in self.n}
        self.events.clear()


STEP_FNS = ("mfvit_adam_step", "mfvit_adam_step_groups", "mfvit_sgd_step", "mfvit_sgd_step_groups", "mfvit_amp_unscale", "mfvit_grad_norm_partials",
            "mfvit_grad_scale")
OPTS = {"AdamW": dict(), "Adam": dict(), "SGD": dict(momentum=0.9)}


def twin(opt_name, single, groups_fn=ref.six_groups, **kw):
    """An optimizer over the nine arena parameters of tests/test_optim_kernels_gpu.py in six groups, with its gradients / states in NaN-guarded
    flat buffers at other phases; two calls give identical twins."""
    from mfvit import optim
    ps, arena, flats = _arena_setup(opt_name)
    cls = getattr(optim, opt_name)
    opt = cls(groups_fn(ps), lr=ref.BASE_LR, single_launch=single, **OPTS[opt_name], **kw)
    for i, p in enumerate(ps):
        if i != FROZEN:
            p.grad = flats["grad"][2][i]
            for k, nm in enumerate(cls.state_names):
                opt.state[p][nm] = flats[f"s{k}"][2][i]
    return opt, ps, arena, flats


def assert_twins_equal(a, b, what):
    (_, _, arena_a, flats_a), (_, _, arena_b, flats_b) = a, b
    assert same_bits(arena_a.flat, arena_b.flat), what
    for k in flats_a:
        assert same_bits(flats_a[k][0], flats_b[k][0]), (what, k)


@pytest.mark.parametrize("opt_name", ["AdamW", "Adam", "SGD"])
def test_single_launch_step_is_the_per_group_step_in_one_call(opt_name, monkeypatch):
    from mfvit.schedules import adjust_learning_rate
    one, per = twin(opt_name, True), twin(opt_name, False)
    assert_twins_equal(one, per, "setup")
    calls = Calls(monkeypatch, STEP_FNS)
    groups_fn, group_fn = ("mfvit_sgd_step_groups", "mfvit_sgd_step") if opt_name == "SGD" else ("mfvit_adam_step_groups", "mfvit_adam_step")
    for s, epoch in enumerate(ref.SCHEDULE_EPOCHS):
        for opt in (one[0], per[0]):
            adjust_learning_rate(opt, epoch, ref.BASE_LR, ref.EPOCHS, ref.WARMUP)
        assert len({g["lr"] for g in one[0].param_groups}) == 6
        start = one[2].flat.clone()
        calls.reset()
        one[0].before_group = lambda gi: calls.events.append(gi)
        one[0].step()
        assert calls.n[groups_fn] == 1 and calls.n[group_fn] == 0
        assert calls.events == [0, 1, 2, 3, 4, 5, groups_fn]                    # every group's hook, in order, before the one launch
        assert calls.args[groups_fn][3] == 6
        calls.reset()
        per[0].step()
        assert calls.n[groups_fn] == 0 and calls.n[group_fn] == 6
        torch.cuda.synchronize()
        assert_twins_equal(one, per, (opt_name, s))
        assert not same_bits(one[2].flat, start) and one[2].intact()
        if opt_name != "SGD":
            assert all(int(one[0].state[p]["step"]) == s + 1 for i, p in enumerate(one[1]) if i != FROZEN)
        for t in (one, per):
            t[3]["grad"][1].mul_(-0.7)
    assert same_bits(one[1][FROZEN].detach(), twin(opt_name, True)[1][FROZEN].detach())            # no gradient: never moved


# ------------------------------------------------------------------------------------------------ 5. GradScaler and clipping on the joined table
@pytest.mark.parametrize("plant", [None, "inf"])
def test_unscale_and_clipping_run_once_over_the_joined_table(plant, monkeypatch):
    from mfvit import optim
    from mfvit.amp import GradScaler
    one, per = twin("AdamW", True), twin("AdamW", False)
    calls = Calls(monkeypatch, STEP_FNS)
    out = []
    for t in (one, per):
        opt, ps = t[0], t[1]
        t[3]["grad"][1].mul_(2.0 ** 10)
        if plant:
            with torch.no_grad():
                ps[8].grad[3] = float("inf")                                   # the last group's last parameter
        scaler = GradScaler(init_scale=2.0 ** 10)
        calls.reset()
        scaler.unscale_(opt)
        total, norms = optim.clip_grad_norm_(opt, 0.5, per_tensor=True)
        n = 1 if t is one else 6
        assert (calls.n["mfvit_amp_unscale"], calls.n["mfvit_grad_norm_partials"], calls.n["mfvit_grad_scale"]) == (n, n, n)
        only = optim.grad_norm(opt)                                            # the norm pass alone
        torch.cuda.synchronize()
        assert calls.n["mfvit_grad_norm_partials"] == 2 * n and calls.n["mfvit_grad_scale"] == n
        out.append((total.clone(), norms.clone(), only.clone(), scaler._found_inf.clone()))
        scaler.step(opt)                                                       # skipped when a gradient overflowed
        assert calls.n["mfvit_adam_step_groups"] == (0 if plant or t is per else 1)
        assert calls.n["mfvit_adam_step"] == (0 if plant or t is one else 6)
    for a, b in zip(*out):
        assert same_bits(a.reshape(-1), b.reshape(-1))
    assert_twins_equal(one, per, "after unscale, clip and step")
    total, _, _, found = out[0]
    assert float(found) == (1.0 if plant else 0.0)
    if plant:
        assert float(total) == float("inf")
    else:
        assert 0.5 < float(total) < float("inf") and float(out[0][2]) < 0.5 * (1 + 1e-5)           # clipped to max_norm


# ------------------------------------------------------------------------------------------------ 6. fallbacks
def test_group_without_gradients_is_left_out(monkeypatch):
    one, per = twin("AdamW", True), twin("AdamW", False)
    calls = Calls(monkeypatch, STEP_FNS)
    for t in (one, per):
        for i in ref.SIX_GROUPS[2] + ref.SIX_GROUPS[4]:                        # group 2 had one live parameter (the other is FROZEN), group 4 one
            t[1][i].grad = None
        t[0].param_groups[0]["lr"] = torch.tensor(t[0].param_groups[0]["lr"])      # a 0-dim tensor lr, which torch allows
        t[0].step()
    torch.cuda.synchronize()
    assert calls.n["mfvit_adam_step_groups"] == 1 and calls.args["mfvit_adam_step_groups"][3] == 4 and calls.n["mfvit_adam_step"] == 4
    assert_twins_equal(one, per, "two groups without gradients")
    fresh = twin("AdamW", True)
    for i in ref.SIX_GROUPS[2] + ref.SIX_GROUPS[4]:
        assert same_bits(one[1][i].detach(), fresh[1][i].detach())
    assert not same_bits(one[1][0].detach(), fresh[1][0].detach())


def test_mixed_step_counters_in_a_group_take_the_per_group_path(monkeypatch):
    one, per = twin("AdamW", True), twin("AdamW", False)
    calls = Calls(monkeypatch, STEP_FNS)
    late = {}
    for t in (one, per):
        late[id(t)] = t[1][1].grad
        t[1][1].grad = None                                                    # parameter 1 of group 0 gets its first gradient one step late
        t[0].step()
    assert calls.n["mfvit_adam_step_groups"] == 1
    calls.reset()
    for t in (one, per):
        t[1][1].grad = late[id(t)]
        t[3]["grad"][1].mul_(-0.7)
        t[0].step()
    torch.cuda.synchronize()
    assert calls.n["mfvit_adam_step_groups"] == 0 and calls.n["mfvit_adam_step"] == 2 * 7           # group 0 in two runs, the others in one
    assert int(one[0].state[one[1][0]]["step"]) == 2 and int(one[0].state[one[1][1]]["step"]) == 1
    assert_twins_equal(one, per, "mixed step counters")
    calls.reset()
    for t in (one, per):
        t[0].step()                                                            # still mixed (2 / 1 -> 3 / 2): the fallback again
    torch.cuda.synchronize()
    assert calls.n["mfvit_adam_step_groups"] == 0
    assert_twins_equal(one, per, "mixed step counters, again")


def test_state_dict_round_trips_with_torch_adamw_and_the_joined_table_is_dropped(monkeypatch):
    one, per = twin("AdamW", True), twin("AdamW", False)
    for t in (one, per):
        t[0].step()
    torch.cuda.synchronize()
    opt, ps = one[0], one[1]
    sd = copy.deepcopy(opt.state_dict())
    assert all(set(g) >= {"lr", "lr_scale", "weight_decay", "betas", "eps"} for g in sd["param_groups"])
    there = torch.optim.AdamW(ref.six_groups(ps), lr=ref.BASE_LR)
    there.load_state_dict(sd)
    assert [g["lr"] for g in there.param_groups] == [g["lr"] for g in opt.param_groups]
    back = copy.deepcopy(there.state_dict())
    assert "joined" in opt._cache()
    opt.load_state_dict(back)
    assert "joined" not in opt._cache()
    calls = Calls(monkeypatch, STEP_FNS)
    for t in (one, per):
        t[3]["grad"][1].mul_(-0.7)
        t[0].step()
    torch.cuda.synchronize()
    assert calls.n["mfvit_adam_step_groups"] == 1
    assert same_bits(one[2].flat, per[2].flat)                                 # the loaded states are copies of the ones the twin kept
    for i, p in enumerate(ps):
        if i != FROZEN:
            q = per[1][i]
            assert int(opt.state[p]["step"]) == 2
            for nm in ("exp_avg", "exp_avg_sq"):
                assert same_bits(opt.state[p][nm], per[0].state[q][nm]), (i, nm)


def test_sam_with_a_single_launch_base_optimizer(monkeypatch):
    from mfvit import optim
    res = []
    calls = Calls(monkeypatch, STEP_FNS)
    for single in (True, False):
        ps, arena, flats = _arena_setup("AdamW")
        kw = dict(single_launch=True) if single else {}
        opt = optim.SAM(ref.six_groups(ps), optim.AdamW, rho=0.05, lr=ref.BASE_LR, **kw)
        assert opt.base_optimizer.single_launch == single and not opt.single_launch and "single_launch" not in opt.param_groups[0]
        for i, p in enumerate(ps):
            if i != FROZEN:
                p.grad = flats["grad"][2][i]
        opt.first_step()
        opt.second_step()
        torch.cuda.synchronize()
        res.append(arena.flat.clone())
    assert calls.n["mfvit_adam_step_groups"] == 1 and calls.n["mfvit_adam_step"] == 6
    assert same_bits(res[0], res[1])


# ------------------------------------------------------------------------------------------------ 7. on a model
def small_model(seed):
    import vits
    torch.manual_seed(seed)
    return vits.vit_small(depth=2, img_size=64, num_classes=3).to(DEV).train()


def two_steps(seed):
    """Two forward / backward / step rounds of a depth-2 encoder under layer decay; returns what the checks need."""
    from mfvit import optim
    from mfvit.losses import cross_entropy
    m = small_model(seed)
    groups = optim.param_groups_layer_decay(m, 1e-3, weight_decay=0.05, layer_decay=ref.LAYER_DECAY)
    opt = optim.AdamW(groups, lr=1e-3, single_launch=True)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    y = torch.tensor([0, 2], device=DEV)
    rec = []
    for _ in range(2):
        out = m(x)
        loss, _ = cross_entropy(out, y)
        loss.backward()
        before = {n: (p.detach().clone(), p.grad.detach().clone()) for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        rec.append((out.detach().clone(), before, {n: p.detach().clone() for n, p in m.named_parameters()}))
    return m, opt, rec


def test_layer_decay_step_on_an_encoder_matches_the_reference_and_reaches_the_shadows():
    from oracle import ref_optim
    m, opt, rec = two_steps(11)
    assert len(opt.param_groups) == 8 and opt.single_launch
    out0, before, after = rec[0]
    names = [n for g in opt.param_groups for n in g["param_names"]]
    assert sorted(names) == sorted(before)                                     # every trainable parameter got a gradient
    worst = 0.0
    for g in opt.param_groups:
        for n in g["param_names"]:
            p0, gr = before[n]
            want = ref_optim.adam_step(p0.cpu(), gr.cpu(), torch.zeros_like(p0).cpu(), torch.zeros_like(p0).cpu(), 1, ref.f32(g["lr"]), ref.f32(0.9),
                                       ref.f32(0.999), ref.f32(1e-8), ref.f32(g["weight_decay"]), decoupled=True)[0]
            e = ref_optim.gate_ratio(after[n], want, ADAM_RTOL, ADAM_ATOL)
            worst = max(worst, e)
            assert e <= 1.0, (n, e)
    print(f"layer-decay AdamW on a depth-2 encoder: worst gate ratio {worst:.2f}")
    assert torch.equal(after["pos_embed"], dict(m.named_parameters())["pos_embed"].detach())
    assert not torch.equal(rec[1][0], out0)                                    # the second forward saw the new weights: the shadows followed
    _, _, again = two_steps(11)
    for (o1, _, a1), (o2, _, a2) in zip(rec, again):
        assert same_bits(o1, o2) and all(same_bits(a1[n], a2[n]) for n in a1)  # the same seed: the same bits


# ------------------------------------------------------------------------------------------------ 8. ModelEma
@pytest.mark.parametrize("warmup", [False, True], ids=["constant", "warmup"])
def test_model_ema_follows_the_float64_recurrence(warmup):
    from mfvit import optim
    m = small_model(13)
    ema = optim.ModelEma(m, decay=0.9, warmup=warmup)
    assert ema.module is not m and not ema.module.training and not any(p.requires_grad for p in ema.module.parameters())
    want = {n: p.detach().double().cpu() for n, p in ema.module.named_parameters()}
    bound = {n: torch.zeros_like(v) for n, v in want.items()}
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        first = ema.module(x).clone()
    for t in range(3):
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):                             # the live model moves (what optimizer.step() does, through the versions)
                p.add_(0.05 * (t + 1) * torch.cos(torch.arange(p.numel(), device=DEV, dtype=torch.float32) + i).view(p.shape))
        d = ref.f32(ref.ema_decay(t, 0.9, warmup))                             # (the decay crosses the C ABI as a float)
        assert ema.decay_at(t) == ref.ema_decay(t, 0.9, warmup)
        ema.update(m)
        torch.cuda.synchronize()
        for n, w in m.named_parameters():
            new, b = ref.ema_ref(want[n], w.detach().cpu(), d)
            want[n], bound[n] = new, bound[n] * d + b
    assert ema.t == 3 and ([ema.decay_at(t) for t in range(3)] == [0.1, 2.0 / 11.0, 0.25] if warmup else ema.decay_at(2) == 0.9)
    for n, p in ema.module.named_parameters():
        err = (p.detach().double().cpu() - want[n]).abs()
        assert bool((err <= bound[n]).all()), (n, float((err - bound[n]).max()))
    assert {n for n, _ in ema.module.named_parameters()} >= {"head.weight", "head.bias", "cls_token", "blocks.1.mlp.fc2.weight"}
    ema.module.eval()
    m.eval()
    with torch.no_grad():
        out_ema, out_live = ema.module(x), m(x)
    assert bool(torch.isfinite(out_ema).all()) and not torch.equal(out_ema, out_live) and not torch.equal(out_ema, first)
    # the state dict round-trips into a fresh average of another model
    other = optim.ModelEma(small_model(14), decay=0.9, warmup=warmup)
    other.load_state_dict(copy.deepcopy(ema.state_dict()))
    assert other.t == 3 and all(torch.equal(a, b) for a, b in zip(other.module.state_dict().values(), ema.module.state_dict().values()))
    with torch.no_grad():
        assert torch.equal(other.module.eval()(x), out_ema)
    with pytest.raises(TypeError, match="flat arena"):
        optim.ModelEma(torch.nn.Linear(4, 3).to(DEV))
