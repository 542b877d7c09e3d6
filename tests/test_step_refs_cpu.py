"""CPU checks behind the single-kernel GPU parity tests of csrc/moco.hip and csrc/optim.hip (tests/test_moco_rowops_gpu.py,
tests/test_optim_kernels_gpu.py):
  1. every float64 restatement those tests compare the kernels with (oracle/ref_moco.py: ce_rows, l2norm_fwd / _bwd, rowdot; oracle/ref_optim.py)
     is pinned to torch itself in float64 - F.cross_entropy / F.normalize + autograd, torch.optim.Adam / AdamW / SGD, the reference's LARS
     (tests/golden/lars_f64.npz: its float64 CPU run; lars.npz: its float32 trajectory) - at 1e-12 relative;
  2. a mutation check: float32 restatements of ce_rows_kernel's head / float4 body / tail sweep and of adam_kernel's vector / pair / tail split
     run over the SAME case matrices as the GPU tests, once as written and once with each index bug planted.  Unmutated they stay under the
     GPU gates in every case (the gates hold for the reference alone); each bug costs at least 100 x the gate in every case that reaches it, and
     every bug is reached: the GPU gates are shown to discriminate before anyone has a GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rng_tensor
from oracle import ref_moco, ref_optim

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = 1e-12


def _gpu_test_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    if bool(torch.isnan(got).any()):
        return float("inf")
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ 1. the float64 restatements against torch
@pytest.mark.parametrize("n,C", [(1, 1), (3, 5), (7, 1025), (300, 9)])
def test_ce_rows_restatement_is_F_cross_entropy(n, C):
    z = rng_tensor(1 + C, (n, C), scale=5.0, dtype=torch.float64).requires_grad_(True)
    t = torch.from_numpy(np.random.Generator(np.random.PCG64(n)).integers(0, C, size=n))
    t[0], t[-1] = C - 1, 0
    loss = F.cross_entropy(z, t)
    loss.backward()
    r_loss, r_lse, r_d = ref_moco.ce_rows(z.detach(), t)
    assert rel(r_loss, loss) < PIN and rel(r_lse, torch.logsumexp(z, dim=1)) < PIN and rel(r_d, z.grad) < PIN
    # float32 inputs are widened, not computed in float32
    z32 = z.detach().float()
    assert rel(ref_moco.ce_rows(z32, t)[2], ref_moco.ce_rows(z32.double(), t)[2]) == 0.0


@pytest.mark.parametrize("n,C", [(1, 1), (5, 2), (4, 65), (130, 100)])
def test_l2norm_and_rowdot_restatements_are_F_normalize_and_its_autograd(n, C):
    x = rng_tensor(20 + C, (n, C), dtype=torch.float64)
    if n >= 4:
        x[1] = 0.0                                                     # y = 0, inv = 1 / eps, dx = dy / eps
        x[2] *= 1e-20 / x[2].norm()                                    # far below eps: the clamp is active, dx = dy / eps up to 1e-16
    x.requires_grad_(True)
    dy = rng_tensor(21 + C, (n, C), dtype=torch.float64)
    y = F.normalize(x, dim=1)
    y.backward(dy)
    r_y, r_inv = ref_moco.l2norm_fwd(x.detach())
    assert rel(r_y, y) < PIN
    assert rel(r_inv, 1.0 / x.detach().norm(dim=1).clamp_min(1e-12)) < PIN
    r_dx = ref_moco.l2norm_bwd(dy, r_y, r_inv)
    rows = (r_dx - x.grad).abs().amax(dim=1) / x.grad.abs().amax(dim=1).clamp_min(1e-300)      # per row: the 1 / eps rows must not hide the others
    assert float(rows.max()) < PIN
    if n >= 4:
        assert torch.equal(r_y[1], torch.zeros(C, dtype=torch.float64)) and float(r_inv[1]) == 1e12 and rel(r_dx[1], dy[1] * 1e12) < PIN
    b = rng_tensor(22 + C, (n, C), dtype=torch.float64)
    assert rel(ref_moco.rowdot(x.detach(), b, 5.0), 5.0 * torch.einsum("nc,nc->n", x.detach(), b)) < PIN


@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD", "SGD_nomomentum"])
def test_optimizer_restatements_are_torch_optim_over_four_steps(name):
    """Four steps; parameter 1 gets its first gradient at step 2 (its own `step` count, its own first-step momentum buffer)."""
    shapes = [(33, 7), (129, 3), (5,)]
    ps = [torch.nn.Parameter(rng_tensor(40 + i, s, dtype=torch.float64)) for i, s in enumerate(shapes)]
    kw = dict(Adam=dict(lr=1e-2, weight_decay=0.1), AdamW=dict(lr=1e-2, weight_decay=0.1, betas=(0.8, 0.99)),
              SGD=dict(lr=0.1, momentum=0.9, weight_decay=0.01), SGD_nomomentum=dict(lr=0.1, weight_decay=0.01))[name]
    opt = getattr(torch.optim, name.split("_")[0])(ps, **kw)
    mine = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), buf=None, step=0) for p in ps]
    for step in range(4):
        for i, (p, s) in enumerate(zip(ps, mine)):
            if i == 1 and step < 2:
                p.grad = None
                continue
            g = rng_tensor(50 + 10 * step + i, p.shape, dtype=torch.float64)
            p.grad = g.clone()
            s["step"] += 1
            if name.startswith("Adam"):
                b1, b2 = kw.get("betas", (0.9, 0.999))
                s["p"], s["m"], s["v"] = ref_optim.adam_step(s["p"], g, s["m"], s["v"], s["step"], kw["lr"], b1, b2, 1e-8, kw["weight_decay"],
                                                             decoupled=name == "AdamW")
            else:
                s["p"], s["buf"] = ref_optim.sgd_step(s["p"], g, s["buf"], kw["lr"], kw.get("momentum", 0.0), kw["weight_decay"],
                                                      first_step=s["step"] == 1)
        opt.step()
        for p, s in zip(ps, mine):
            assert rel(s["p"], p) < PIN, (name, step)
    for p, s in zip(ps, mine):
        st = opt.state[p]
        if name.startswith("Adam"):
            assert rel(s["m"], st["exp_avg"]) < PIN and rel(s["v"], st["exp_avg_sq"]) < PIN and int(st["step"]) == s["step"]
        elif name == "SGD":
            assert rel(s["buf"], st["momentum_buffer"]) < PIN
        else:
            assert s["buf"] is None                                    # momentum == 0: no buffer is ever made or touched


def test_lars_restatement_is_the_reference_lars(golden):
    """lars_f64.npz: the reference's LARS run in float64 on the CPU, parameters and `mu` after each of three steps (oracle/make_golden.py::
    golden_lars_f64) - a 1-D tensor, a zero parameter, a gradient of -wd * p.  lars.npz is the reference's float32 trajectory: the float64
    restatement, its state rounded to float32 after each step, follows it to float32 rounding (the bound of tests/test_oracle_golden.py::test_lars_trajectory)."""
    g = golden("lars_f64.npz")
    shapes = [(40, 30), (37,), (4, 3), (3, 2), (129, 3)]
    assert [str(s) for s in shapes] == list(g["shapes"])
    kw = dict(lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), momentum=float(g["momentum"]), trust_coefficient=float(g["trust"]))
    ps = [rng_tensor(430 + i, s, dtype=torch.float64) for i, s in enumerate(shapes)]
    ps[3] = torch.zeros_like(ps[3])
    mus = [torch.zeros_like(p) for p in ps]
    for step in range(3):
        for i in range(len(ps)):
            gr = rng_tensor(440 + 10 * step + i, shapes[i], dtype=torch.float64)
            if step == 1 and i == 2:
                gr = -kw["weight_decay"] * ps[i]
            ps[i], mus[i] = ref_optim.lars_step(ps[i], gr, mus[i], **kw)
            assert rel(ps[i], torch.from_numpy(g[f"p{i}.step{step}"])) < PIN, (i, step)
            assert rel(mus[i], torch.from_numpy(g[f"mu{i}.step{step}"])) < PIN or float(mus[i].abs().max()) == 0.0, (i, step)
    # a flattened parameter with its ndim handed in is the same tensor
    a, b = ref_optim.lars_step(ps[0].flatten(), ps[0].flatten() * 0.3, mus[0].flatten(), ndim=2, **kw)
    a2, b2 = ref_optim.lars_step(ps[0], ps[0] * 0.3, mus[0], **kw)
    assert torch.equal(a, a2.flatten()) and torch.equal(b, b2.flatten())
    g32 = golden("lars.npz")
    shapes = [(6, 5), (5,), (4, 3), (3, 2)]
    kw = dict(lr=float(g32["lr"]), weight_decay=float(g32["weight_decay"]), momentum=float(g32["momentum"]), trust_coefficient=float(g32["trust"]))
    ps = [rng_tensor(400 + i, s) for i, s in enumerate(shapes)]
    ps[3] = torch.zeros_like(ps[3])
    mus = [torch.zeros_like(p) for p in ps]
    for step in range(3):
        for i in range(len(ps)):
            gr = rng_tensor(410 + 10 * step + i, shapes[i])
            if step == 1 and i == 2:
                gr = (-kw["weight_decay"] * ps[i]).float()
            ps[i], mus[i] = (t.float() for t in ref_optim.lars_step(ps[i], gr, mus[i], **kw))      # float32 state, as in the recorded run: -wd * p cancels exactly
            torch.testing.assert_close(ps[i].double(), torch.from_numpy(g32[f"p{i}.step{step}"]), rtol=2e-6, atol=1e-7)


def test_amp_unscale_restatement():
    g = torch.tensor([1.0, -3.4028235e38, 3.4028235e38, 0.0], dtype=torch.float32)
    out, flag = ref_optim.amp_unscale(g, 2.0 ** -12)
    assert not flag and torch.equal(out.float(), g * 2.0 ** -12)
    for bad in (float("inf"), -float("inf"), float("nan")):
        h = g.clone()
        h[2] = bad
        assert ref_optim.amp_unscale(h, 2.0 ** -12)[1]
    assert not ref_optim.amp_unscale(torch.tensor([3e38]), 4.0)[1]       # finite before the scaling: not flagged, whatever the product is


# ------------------------------------------------------------------------------------------------ 2. mutation checks
@pytest.mark.parametrize("C", ref_moco.CE_C)
def test_ce_rows_gate_separates_the_right_sweep_from_index_bugs(C):
    gpu = _gpu_test_module("test_moco_rowops_gpu")
    gate = gpu.CE_GATE
    assert gate <= 2e-5
    pool = rng_tensor(9000 + C, (max(ref_moco.CE_N) if C <= 4097 else ref_moco.CE_N_WIDE, C), scale=5.0)
    hits = {}
    floor, reached, weakest = 0.0, {m: 0 for m in ref_moco.CE_MUTATIONS}, {m: float("inf") for m in ref_moco.CE_MUTATIONS}
    for case in ref_moco.ce_cases(C):
        z, t = ref_moco.ce_case_inputs(case, pool, hits.setdefault(case["off"], set()))
        assert float((z - z.max(dim=1, keepdim=True).values).min()) >= -40.0
        r_loss, r_lse, r_d = ref_moco.ce_rows(z, t)

        def errs(out):
            e = [rel(out[0], r_loss), rel(out[1], r_lse)]
            if case["mode"] != "null":
                e.append(rel(out[2], r_d))
            return max(e)
        e0 = errs(ref_moco.ce_rows_sweep_f32(z, t, case))
        floor = max(floor, e0)
        assert e0 < gate, (case, e0)                                    # the reference alone: float32 with exact exp / log is under the gate
        for m in ref_moco.CE_MUTATIONS:
            out = ref_moco.ce_rows_sweep_f32(z, t, case, mutate=m)
            if not out[3]:
                continue
            reached[m] += 1
            e = errs(out)
            weakest[m] = min(weakest[m], e)
            assert e >= 100 * gate, (case, m, e)
    print(f"ce_rows C={C}: float32 restatement vs float64 max {floor:.2e} (gate {gate:.0e}); mutations reached {reached}, weakest error {weakest}")
    assert all(reached[m] > 0 for m in reached) or C < 4, reached
    if C < 4:      # no float4 body can exist: only the scalar segments are there to lose
        assert reached["skip_head"] > 0 and reached["skip_tail"] > 0, reached


def test_ce_rows_case_matrix_covers_every_target_class_and_both_store_paths():
    """The same assertions the GPU test makes from the phase arithmetic, here for the whole matrix at once (no kernel needed)."""
    for C in ref_moco.CE_C:
        ns = set()
        for off in range(4):
            want, dvec = set(), set()
            for case in ref_moco.ce_cases(C):
                if case["off"] != off:
                    continue
                ns.add(case["n"])
                head, tail0 = ref_moco.ce_row_split(C, case["n"], off, case["ld"])
                for h, t0 in set(zip(head.tolist(), tail0.tolist())):
                    want |= set(ref_moco.ce_target_classes(C, h, t0))
                if case["mode"] != "null":
                    dvec |= set(ref_moco.ce_row_dvec(case).tolist())
            assert {"col0", "last"} <= want
            assert dvec == {True, False}, (C, off)
            if C >= 8:
                assert {"head0", "head1", "head2", "tail0", "tail1", "tail2", "first.x", "first.w", "final.x", "final.w"} <= want, (C, off, want)
        assert ns == (set(ref_moco.CE_N) if C <= 4097 else {ref_moco.CE_N_WIDE}), (C, ns)


def _adam_inputs(count, seed):
    p, g = rng_tensor(seed, (count,)), rng_tensor(seed + 1, (count,))
    m, v = rng_tensor(seed + 2, (count,), scale=0.1), rng_tensor(seed + 3, (count,), scale=0.1).abs()
    return p, g, m, v


def test_adam_gate_separates_the_right_split_from_index_bugs():
    gpu = _gpu_test_module("test_optim_kernels_gpu")
    rtol, atol = gpu.ADAM_RTOL, gpu.ADAM_ATOL
    assert (rtol, atol) == (2e-6, 2e-7)
    hyper = gpu.ADAM_HYPER
    reached = {m: 0 for m in ref_optim.ADAM_MUTATIONS}
    paths, worst = set(), 0.0
    for count in ref_optim.ADAM_COUNTS + (3 * gpu.CHUNK_ROW + 5,):
        rows = [min(gpu.CHUNK_ROW, count - a) for a in range(0, count, gpu.CHUNK_ROW)]
        for align in ref_optim.ADAM_ALIGN:
            for step in gpu.ADAM_STEPS:
                for decoupled in (False, True):
                    p, g, m, v = _adam_inputs(count, 7000 + count % 997)
                    if step == 1:
                        m, v = torch.zeros_like(m), torch.zeros_like(v)
                    ref = ref_optim.adam_step(p, g, m, v, step, decoupled=decoupled, **hyper)
                    for mutate in (None,) + ref_optim.ADAM_MUTATIONS:
                        out, hit, a = [[], [], []], False, 0
                        for n in rows:          # (a table row per CHUNK elements: the split restarts in every row)
                            o = ref_optim.adam_split_f32(p[a:a + n], g[a:a + n], m[a:a + n], v[a:a + n], align == "aligned", step,
                                                         decoupled=decoupled, mutate=mutate, **hyper)
                            for k in range(3):
                                out[k].append(o[k])
                            hit |= o[3]
                            if mutate is None:
                                paths |= set(ref_optim.adam_path_of(n, align == "aligned").tolist())
                            a += n
                        e = max(ref_optim.gate_ratio(torch.cat(out[k]), ref[k], rtol, atol) for k in range(3))
                        if mutate is None:
                            worst = max(worst, e)
                            assert e <= 1.0, (count, align, step, decoupled, e)
                        elif hit:
                            reached[mutate] += 1
                            assert e >= 100.0, (count, align, step, decoupled, mutate, e)
    print(f"adam split: float32 restatement at most {worst:.2f} of the gate; mutations reached {reached}")
    assert all(v > 0 for v in reached.values()), reached
    assert paths == {0, 1, 2, 3}, paths                                 # vector single, vector pair, tail, scalar fallback
