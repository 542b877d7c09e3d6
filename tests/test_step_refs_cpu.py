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


# ------------------------------------------------------------------------------------------------ 3. the BatchNorm entry points (tests/test_bn_edges_gpu.py)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "noaffine"])
@pytest.mark.parametrize("n,C", [(1, 3), (2, 1), (17, 5), (33, 68)])
def test_bn_restatements_are_F_batch_norm_and_its_autograd_in_training(n, C, affine, relu):
    x = rng_tensor(40 + n + C, (n, C), scale=2.0, dtype=torch.float64) + 0.5
    x[:, 0] = ref_moco.BN_CONST                                          # a constant column: var = 0
    x.requires_grad_(True)
    dy = rng_tensor(41 + n + C, (n, C), dtype=torch.float64)
    w = (1 + 0.1 * rng_tensor(42 + C, (C,), dtype=torch.float64)).requires_grad_(True) if affine else None
    b = (0.1 * rng_tensor(43 + C, (C,), dtype=torch.float64)).requires_grad_(True) if affine else None
    rm0, rv0 = rng_tensor(44 + C, (C,), dtype=torch.float64), rng_tensor(45 + C, (C,), dtype=torch.float64).abs() + 0.5
    for eps, mom in ((1e-5, 0.1), (1e-3, 0.37)):
        for t in (x, w, b):
            if t is not None:
                t.grad = None
        rm, rv = rm0.clone(), rv0.clone()
        if n > 1:
            y = F.batch_norm(x, rm, rv, w, b, training=True, momentum=mom, eps=eps)
        else:                      # torch refuses one value per channel in training; SyncBatchNorm's arithmetic at N = 1 is var = 0, biased in the running variance
            y = (x - x.detach()) / (0.0 + eps) ** 0.5 * (w if affine else 1.0) + (b if affine else 0.0)
            rm, rv = (1 - mom) * rm + mom * x.detach()[0], (1 - mom) * rv
        out = torch.relu(y) if relu else y
        out.backward(dy)
        xd = x.detach()
        mean_p, m2_p = ref_moco.bn_stats(xd)
        mean, invstd, r_rm, r_rv = ref_moco.bn_combine(mean_p[None], m2_p[None], torch.tensor([float(n)]), eps, mom, rm0, rv0)
        assert rel(mean, xd.mean(0)) < PIN and rel(r_rm, rm) < PIN and rel(r_rv, rv) < PIN
        wd, bd = (w.detach(), b.detach()) if affine else (None, None)
        r_y = ref_moco.bn_apply(xd, mean, invstd, wd, bd, relu)
        assert rel(r_y, out) < PIN
        s1, s2 = ref_moco.bn_bwd_sums(dy, xd, r_y, mean, invstd, relu)
        dx = ref_moco.bn_bwd_apply(dy, xd, r_y, mean, invstd, wd, relu, s1, s2, 1.0 / n)
        if n > 1:
            assert rel(dx, x.grad) < 1e-9                                # (the constant column: differences of terms invstd = 1 / sqrt(eps) larger)
            if affine:
                assert rel(s1, b.grad) < PIN and rel(s2, w.grad) < PIN
        else:
            assert not bool(dx.any())


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "noaffine"])
def test_bn_restatements_are_F_batch_norm_and_its_autograd_in_eval(affine):
    """eval mode as mfvit/mlp.py runs it: mean = running mean, invstd = rsqrt(running var + eps), and the sums of the backward zeroed."""
    n, C, eps = 9, 6, 1e-5
    x = rng_tensor(50, (n, C), dtype=torch.float64).requires_grad_(True)
    dy = rng_tensor(51, (n, C), dtype=torch.float64)
    w = (1 + 0.1 * rng_tensor(52, (C,), dtype=torch.float64)) if affine else None
    b = 0.1 * rng_tensor(53, (C,), dtype=torch.float64) if affine else None
    rm, rv = rng_tensor(54, (C,), dtype=torch.float64), rng_tensor(55, (C,), dtype=torch.float64).abs() + 0.5
    y = torch.relu(F.batch_norm(x, rm, rv, w, b, training=False, eps=eps))
    y.backward(dy)
    invstd = 1.0 / torch.sqrt(rv + eps)
    r_y = ref_moco.bn_apply(x.detach(), rm, invstd, w, b, True)
    zero = torch.zeros(C, dtype=torch.float64)
    assert rel(r_y, y) < PIN
    assert rel(ref_moco.bn_bwd_apply(dy, x.detach(), r_y, rm, invstd, w, True, zero, zero, 1.0 / n), x.grad) < PIN


def test_bn_relu_mask_passes_positive_values_only():
    y = torch.tensor([[1.0, 0.0, -0.0, -2.0, float("nan"), 1e-30]])
    assert ref_moco.bn_masked(torch.ones(1, 6), y, True).tolist() == [[1.0, 0.0, 0.0, 0.0, 0.0, 1.0]]
    assert ref_moco.bn_masked(torch.ones(1, 6), y, False).tolist() == [[1.0] * 6]
    for prec in ref_moco.BN_DTYPES:                                      # the hand-built y of the case matrix holds all five kinds
        yh = ref_moco.bn_case_inputs(prec, 5, 7, "plain")[2].float()
        assert bool((yh > 0).any()) and bool((yh < 0).any()) and bool(torch.isnan(yh).any())
        zeros = yh[yh == 0]
        assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())


def test_bn_combine_restatement_is_the_statistics_of_the_concatenated_batch_and_skips_empty_ranks():
    C = 5
    for name, counts in ref_moco.BN_COMBINE_COUNTS.items():
        g = torch.Generator().manual_seed(len(counts))
        parts = [torch.randn(k, C, generator=g, dtype=torch.float64) * 3 + w for w, k in enumerate(counts)]
        st = [ref_moco.bn_stats(p) for p in parts]
        means, m2s, cnt = torch.stack([s[0] for s in st]), torch.stack([s[1] for s in st]), torch.tensor(counts, dtype=torch.float64)
        allx = torch.cat(parts)
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        F.batch_norm(allx, rm, rv, training=True, momentum=0.37, eps=1e-3)
        want = (allx.mean(0), 1.0 / torch.sqrt(allx.var(0, unbiased=False) + 1e-3), rm, rv)
        got = ref_moco.bn_combine(means, m2s, cnt, 1e-3, 0.37, torch.zeros(C), torch.ones(C))
        assert all(rel(a, b) < PIN for a, b in zip(got, want)), name
        # the rank-by-rank statement of the same (bn_chan_combine) agrees
        chan = ref_moco.bn_chan_combine(torch.cat([torch.cat([m, q, k[None]]) for m, q, k in zip(means, m2s, cnt)]), C, 1e-3)
        assert rel(chan[0], got[0]) < PIN and rel(chan[2], got[1]) < PIN
        for pos in (0, len(counts) // 2, len(counts)):                   # an empty rank with garbage in it changes nothing, wherever it stands
            m9 = torch.cat([means[:pos], torch.full((1, C), 1e30, dtype=torch.float64), means[pos:]])
            q9 = torch.cat([m2s[:pos], torch.full((1, C), 7.0, dtype=torch.float64), m2s[pos:]])
            k9 = torch.cat([cnt[:pos], torch.zeros(1, dtype=torch.float64), cnt[pos:]])
            again = ref_moco.bn_combine(m9, q9, k9, 1e-3, 0.37, torch.zeros(C), torch.ones(C))
            assert all(torch.equal(a, b) for a, b in zip(again, got)), (name, pos)
            f32 = ref_moco.bn_combine_f32(m9, q9, k9, 1e-3)
            assert all(torch.equal(a, b) for a, b in zip(f32, ref_moco.bn_combine_f32(means, m2s, cnt, 1e-3))), (name, pos)


def test_bn_float32_floors_stay_under_a_quarter_of_the_gates():
    """The float32 restatements of the two-pass statistics and of the combine over the case matrix of tests/test_bn_edges_gpu.py, against float64: what
    float32 itself costs, before any kernel.  A quarter of the gate at most, or the input is badly chosen; the figures stand above the gates there."""
    gpu = _gpu_test_module("test_bn_edges_gpu")
    assert gpu.STAT_GATE <= 5e-5 and gpu.COMBINE_GATE <= 2e-5
    assert all(gpu.OUT_GATE[p] <= t for p, t in (("f32", 5e-5), ("fp16", 2e-3), ("bf16", 1.6e-2)))
    for prec, dt in ref_moco.BN_DTYPES.items():
        floor, col, one_pass, out, dx_floor, dx2_own, dx2_terms = 0.0, 0.0, float("inf"), 0.0, 0.0, 0.0, 0.0
        for C in ref_moco.BN_C:
            for n in ref_moco.BN_N:
                for family in ("plain", "edge"):
                    x, dy, y, gamma, beta = ref_moco.bn_case_inputs(prec, n, C, family)
                    (mu, q), (r_mu, r_q) = ref_moco.bn_stats_f32(x), ref_moco.bn_stats(x)
                    floor = max(floor, rel(mu, r_mu), rel(q, r_q))
                    if family == "edge" and C > 1 and n > 1:               # the mean >> std column on its own scale, and what one pass would give
                        col = max(col, float((mu[1] - r_mu[1]).abs() / r_mu[1].abs()), float((q[1] - r_q[1]).abs() / r_q[1].clamp_min(1e-30)))
                        if n >= 15:
                            q1 = ref_moco.bn_stats_f32(x, one_pass=True)[1]
                            one_pass = min(one_pass, float((q1[1] - r_q[1]).abs() / r_q[1]))
                    r_mean, r_is, _, _ = ref_moco.bn_combine(r_mu[None], r_q[None], torch.tensor([float(n)]))
                    r_y = ref_moco.bn_apply(x, r_mean, r_is, gamma, beta, True)
                    if float(r_y.abs().max()) > 0:
                        out = max(out, rel(r_y.to(dt), r_y))
                    # dx in float32 from float32-rounded statistics and sums, before the rounding to the element type
                    m32, i32 = r_mean.float(), r_is.float()
                    s1, s2 = (t.float() for t in ref_moco.bn_bwd_sums(dy, x, y, m32, i32, True))
                    args = (dy, x, y, m32, i32, gamma, True, s1, s2, float(np.float32(1.0 / n)))
                    r_dx, dx32 = ref_moco.bn_bwd_apply(*args), ref_moco.bn_bwd_apply_f32(*args)
                    if n == 2:
                        dx2_own = max(dx2_own, rel(dx32, r_dx))
                        dx2_terms = max(dx2_terms, float((dx32.double() - r_dx).abs().max()) / max(ref_moco.bn_bwd_apply_terms(*args), 1e-30))
                    elif n > 2:
                        dx_floor = max(dx_floor, rel(dx32, r_dx))
        print(f"bn statistics[{prec}]: float32 two-pass restatement vs float64 max {floor:.2e}; mean >> std column (ratio {ref_moco.BN_RATIO[prec]:g}) "
              f"{col:.2e} on its own scale, one pass at least {one_pass:.2e} (gate {gpu.STAT_GATE:.0e}); y rounded to {prec} {out:.2e} (gate {gpu.OUT_GATE[prec]:.0e})")
        print(f"bn dx[{prec}] in float32, before its rounding to {prec}: n >= 15 max {dx_floor:.2e}; n = 2 {dx2_own:.2e} of its own size (it vanishes identically), "
              f"{dx2_terms:.2e} of its terms")
        # the mean >> std column stays under a quarter of the gate; the whole matrix under the gate and under a quarter of the ceiling (the kernels
        # are no less exact than this restatement, so a gate of 4 x what they measure cannot be 4 x this floor as well)
        assert col < gpu.STAT_GATE / 4 and floor < min(gpu.STAT_GATE, 5e-5 / 4)
        assert max(dx_floor, dx2_terms) < 5e-5 / 4 < dx2_own
        assert out < gpu.OUT_GATE[prec] / 4 or prec != "f32"               # (the 16-bit outputs: their rounding IS the error; see OUT_GATE)
        if prec == "f32":
            assert one_pass > 10 * gpu.STAT_GATE                           # the second pass earns its keep: one pass is told apart by the gate
    worst = 0.0
    for C in (1, 5, 256, 257, 1028):
        for counts in ref_moco.BN_COMBINE_COUNTS.values():
            means, m2s, cnt = ref_moco.bn_combine_inputs(C, counts)
            for eps in (1e-5, 1e-3):
                mu, invstd, unb = ref_moco.bn_combine_f32(means, m2s, cnt, eps)
                r = ref_moco.bn_combine(means, m2s, cnt, eps, 0.1, torch.zeros(C), torch.zeros(C))
                worst = max(worst, rel(mu, r[0]), rel(invstd, r[1]), rel(0.1 * unb.double(), r[3]))
    print(f"bn combine: float32 rank-by-rank restatement vs float64 max {worst:.2e} (gate {gpu.COMBINE_GATE:.0e})")
    assert worst < min(gpu.COMBINE_GATE, 2e-5 / 4)                         # (the kernel measures what this restatement does: the gate is 4 x this floor)


# ------------------------------------------------------------------------------------------------ 4. the small cross entropies (tests/test_ce_small_gpu.py)
def test_ce_small_float32_floor_and_case_matrix():
    """ce_small_kernel restated in float32 with exact exp / log over the case matrix of tests/test_ce_small_gpu.py, by that test's own measures: the
    floor of CE_SMALL_GATE.  And the matrix holds what it says: targets in column 0 and C - 1, tie rows whose first maximum is column C // 3,
    saturated rows with a tiny loss beside rows with a large one."""
    gpu = _gpu_test_module("test_ce_small_gpu")
    assert all(v <= 2e-5 for v in gpu.CE_SMALL_GATE.values())
    floor = dict(loss=0.0, dlogits=0.0)
    for C in ref_moco.CE_SMALL_C:
        for B in ref_moco.CE_SMALL_B:
            for scale in ref_moco.CE_SMALL_SCALES:
                z, t = ref_moco.ce_small_case(B, C, scale)
                zd = z.double().requires_grad_(True)
                rows = F.cross_entropy(zd, t, reduction="none")
                rows.mean().backward()
                if B > 1:
                    assert int(t[0]) == 0 and int(t[-1]) == C - 1 and int(z.max(1)[1][1]) == C // 3 and (C == 1 or float(z[1, C // 3]) == float(z[1, C - 1]))
                if scale > 1 and C > 2 and B > 1000:
                    assert float(rows.detach().min()) < 1e-6 and float(rows.detach().max()) > 50.0
                loss, d = ref_moco.ce_small_f32(z, t)
                e = gpu.errors(loss, d, float(rows.detach().mean()), zd.grad, float(rows.detach().max()), scale, B)
                floor = {k: max(floor[k], e[k]) for k in floor}
    print(f"small cross entropy: float32 restatement vs float64 max loss {floor['loss']:.2e} dlogits {floor['dlogits']:.2e} (gates {gpu.CE_SMALL_GATE})")
    assert all(v < min(gpu.CE_SMALL_GATE[k], 2e-5 / 4) for k, v in floor.items())
