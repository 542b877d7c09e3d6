"""CPU side of the fusion edge tests (tests/test_fusion_edges_gpu.py):
  * the general float64 restatement oracle.ref_fusion.fus_ex_forward / exchange_ex is pinned to the reference's own outputs and gradients at every
    fusion golden (tests/golden/fusion_ex_*.npz: heads 3, 6 and 12, dim 384 / 768, depth 1 - 3, both pools; fusion_e2e, fusion_exchange), so
    the edge tests' oracle is pinned to the reference project and not only to itself;
  * the float32 floor of every edge case: the same restatement evaluated in float32 on the CPU against float64, per quantity class - printed,
    appended to the fusion parity report (test_fusion_gpu.REPORT), and asserted to stay under the gates of tests/fusion_edges_ref.py;
  * the host-side argument checks of the C ABI (num_classes 1 .. 64, tokens 2 .. T_max): MFVIT_EINVAL before any HIP call, 0 from the queries."""
import os

import pytest
import torch

import fusion_edges_ref as fe
from conftest import check_sampled, rng_tensor
from oracle import ref_fusion, ref_vit
from test_fusion_gpu import REPORT     # where the fusion tests log their measured errors

F64 = torch.float64
FUS_CASES = ["d384_h3_L2_cls_M1", "d384_h3_L1_mean_M1", "d768_h3_L1_cls_M1", "d768_h12_L2_mean_M2", "d384_h6_L3_cls_M1", "d384_h3_L2_cls_M1_T577"]
EINVAL = -22


def log(msg):
    print(msg)
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")


def golden_state(keys, seed, D, C):
    """tools/make_fusion_ex_golden.py::seeded_state from the key list alone (the shapes follow from the names)."""
    sd = {}
    for i, k in enumerate(keys):
        k = str(k)
        if k.startswith("mlp_head_"):
            shape = (C, D) if k.endswith("weight") else (C,)
        else:
            shape = (D, D) if k.endswith(("wq.weight", "wk.weight", "wv.weight", "proj.weight")) else (D,)
        if len(shape) == 2:
            sd[k] = rng_tensor(seed * 1000 + i, shape, 0.05, F64)
        elif k.endswith("bias"):
            sd[k] = rng_tensor(seed * 1000 + i, shape, 0.1, F64)
        else:
            sd[k] = 1.0 + rng_tensor(seed * 1000 + i, shape, 0.1, F64)
    return sd


@pytest.mark.parametrize("case", FUS_CASES)
def test_restatement_matches_the_reference_at_every_fusion_ex_golden(golden, case):
    g = golden(f"fusion_ex_{case}.npz")
    D, H, L, M, B, T, C, seed = (int(g[k]) for k in ("dim", "heads", "depth", "msd", "B", "T", "C", "seed"))
    pool = str(g["pool"])
    p = {k: v.requires_grad_(True) for k, v in golden_state(g["keys"], seed, D, C).items()}
    fc = rng_tensor(seed + 1, (B, T, D), dtype=F64).requires_grad_(True)
    fe_ = rng_tensor(seed + 2, (B, T, D), dtype=F64).requires_grad_(True)
    hw = [rng_tensor(seed + 3 + i, (C, D), 0.05, F64).requires_grad_(True) for i in range(2)]
    hb = [rng_tensor(seed + 5 + i, (C,), 0.1, F64).requires_grad_(True) for i in range(2)]
    fused, xc, xe = ref_fusion.fus_ex_forward(p, fc, fe_, H, L, pool, M, hw[0], hb[0], hw[1], hb[1])
    r = [rng_tensor(seed + 7 + i, (B, C), dtype=F64) for i in range(3)]
    loss = (fused * r[0]).sum() + (xc * r[1]).sum() + (xe * r[2]).sum()
    loss.backward()
    for name, t in (("fused", fused), ("x_cxr", xc), ("x_enh", xe), ("loss", loss)):
        torch.testing.assert_close(t.detach(), torch.from_numpy(g[name]), rtol=1e-9, atol=1e-10)
    for k, v in p.items():
        if f"nograd.{k}" in g:
            assert v.grad is None, k
        else:
            check_sampled(g, "d." + k, v.grad)
    for i, s in enumerate(("cxr", "enh")):
        torch.testing.assert_close(hw[i].grad, torch.from_numpy(g[f"d.hw_{s}"]), rtol=1e-9, atol=1e-10)
        torch.testing.assert_close(hb[i].grad, torch.from_numpy(g[f"d.hb_{s}"]), rtol=1e-9, atol=1e-10)
    check_sampled(g, "d.f_cxr", fc.grad)
    check_sampled(g, "d.f_enh", fe_.grad)


@pytest.mark.parametrize("case", ["d768_h3_L1", "d768_h3_L2"])
def test_exchange_restatement_matches_the_reference_golden(golden, case):
    g = golden(f"fusion_ex_xch_{case}.npz")
    D, H, L, B, T, seed = (int(g[k]) for k in ("dim", "heads", "depth", "B", "T", "seed"))
    pre = "multi_scale_transformers.0."
    p = {pre + k: v.requires_grad_(True) for k, v in golden_state(g["keys"], seed, D, 3).items()}
    xs = rng_tensor(seed + 1, (B, T, D), dtype=F64).requires_grad_(True)
    xl = rng_tensor(seed + 2, (B, T, D), dtype=F64).requires_grad_(True)
    xs_o, xl_o = ref_fusion.exchange_ex(p, xs, xl, H, L)
    r = [rng_tensor(seed + 3 + i, (B, T, D), dtype=F64) for i in range(2)]
    ((xs_o * r[0]).sum() + (xl_o * r[1]).sum()).backward()
    check_sampled(g, "xs_out", xs_o)
    check_sampled(g, "xl_out", xl_o)
    check_sampled(g, "d.xs", xs.grad)
    check_sampled(g, "d.xl", xl.grad)
    for k, v in p.items():
        check_sampled(g, "d." + k[len(pre):], v.grad)


def test_restatement_matches_fusion_exchange_and_e2e_goldens(golden):
    g = golden("fusion_exchange.npz")
    fp = ref_fusion.seeded_fusion_ex_params(int(g["seed_params"]), dtype=F64)
    xs, xl = rng_tensor(int(g["seed_xs"]), (2, 197, 384), dtype=F64), rng_tensor(int(g["seed_xl"]), (2, 197, 384), dtype=F64)
    xs_o, xl_o = ref_fusion.exchange_ex(fp, xs, xl)
    check_sampled(g, "xs_out", xs_o)
    check_sampled(g, "xl_out", xl_o)
    g = golden("fusion_e2e.npz")
    fp = {k: v.requires_grad_(True) for k, v in ref_fusion.seeded_fusion_ex_params(int(g["seed_params"]), dtype=F64).items()}
    depth = int(g["vit_depth"])
    vc = ref_vit.seeded_params(int(g["seed_vit_cxr"]), num_classes=3, depth=depth, dtype=F64)
    ve = ref_vit.seeded_params(int(g["seed_vit_enh"]), num_classes=3, depth=depth, dtype=F64)
    ic, ie = rng_tensor(int(g["seed_img_cxr"]), (2, 3, 224, 224), dtype=F64), rng_tensor(int(g["seed_img_enh"]), (2, 3, 224, 224), dtype=F64)
    fused, xc, xe = ref_fusion.fus_ex_forward(fp, ref_vit.features3d(vc, ic), ref_vit.features3d(ve, ie), 3, 1, "cls", 1, vc["head.weight"],
                                              vc["head.bias"], ve["head.weight"], ve["head.bias"])
    loss = torch.nn.functional.cross_entropy(fused + xc + xe, torch.from_numpy(g["target"]))
    for name, t in (("fused", fused), ("x_cxr", xc), ("x_enh", xe), ("loss", loss)):
        torch.testing.assert_close(t.detach(), torch.from_numpy(g[name]), rtol=1e-9, atol=1e-10)
    loss.backward()
    for k, v in fp.items():
        check_sampled(g, "d." + k, v.grad)


# ------------------------------------------------------------------------------------------------------------ float32 floors
def floor_of(c):
    inp = fe.make_inputs(c)
    f32 = fe.evaluate(c, inp, torch.float32)
    if c.stress == "nan":   # the NaN sample is compared on neither side; the batch-summed gradients are NaN in the oracle itself
        return fe.errors(f32, fe.oracle(c), c.H, samples=[b for b in range(c.B) if b != fe.STRESS_SAMPLE], skip_params=True)
    return fe.errors(f32, fe.oracle(c), c.H)


@pytest.mark.parametrize("group", ["batch", "classes", "tokens", "lds", "stress"])
def test_float32_floor_stays_under_every_gate(group):
    cases = dict(batch=fe.batch_cases, classes=fe.class_cases, tokens=fe.token_cases, lds=fe.lds_cases, stress=fe.stress_cases)[group]()
    for ill in (False, True):        # (the mean_1e3 stress has gates of its own: fusion_edges_ref.GATES_MEAN_1E3)
        total, worst, n = {}, {}, 0
        for c in cases:
            if (c.stress == "mean_1e3") != ill:
                continue
            n += 1
            for q, e in floor_of(c).items():
                if e > total.get(q, -1.0):
                    total[q], worst[q] = e, c
        if n:
            log(f"fusion edges, float32 CPU floor vs float64 [{group}{' mean_1e3' if ill else ''}, {n} cases]: " +
                "  ".join(f"{q} {total[q]:.2e} ({fe.case_id(worst[q])})" for q in fe.QUANTITIES if q in total))
            fe.check_gates(total, f"float32 floor [{group}]", worst["out"])


@pytest.mark.parametrize("bare", [False, True], ids=["prenorm_xattn", "xattn"])
def test_float32_floor_of_the_standalone_cross_attention_stays_under_its_gates(bare):
    total, worst = {}, {}
    for D, H, B, T in fe.XATTN_GRID:
        xi = fe.xattn_inputs(D, H, B, T, bare)
        for q, e in fe.errors(fe.xattn_evaluate(xi, torch.float32), fe.xattn_evaluate(xi), H).items():
            if e > total.get(q, -1.0):
                total[q], worst[q] = e, f"d{D}_h{H}_B{B}_T{T}"
    log(f"fusion edges, float32 CPU floor vs float64 [{'xattn' if bare else 'prenorm_xattn'}, {len(fe.XATTN_GRID)} cases]: " +
        "  ".join(f"{q} {total[q]:.2e} ({worst[q]})" for q in fe.QUANTITIES if q in total))
    fe.check_gates(total, "float32 floor [stand-alone cross-attention]", gates=fe.GATES_XATTN)


# ------------------------------------------------------------------------------------------------------------ host checks
def _queries(cfg, L, pm):
    from mfvit import _lib
    lib = _lib.lib()
    q = [lib.mfvit_fusion_ex_param_count(cfg, L, pm), lib.mfvit_fusion_ex_workspace_bytes(cfg, L, pm)]
    if L == 1 and pm == 0:
        q += [lib.mfvit_fusion_param_count(cfg), lib.mfvit_fusion_workspace_bytes(cfg)]
    return q


FAKE = 0x1000     # never dereferenced: only sent with class / token counts that the entry points have always refused on the host


def _calls(cfg, L, pm):
    from mfvit import _lib
    lib = _lib.lib()
    rc = [lib.mfvit_fusion_ex_forward(cfg, L, pm, *([FAKE] * 11), None), lib.mfvit_fusion_ex_backward(cfg, L, pm, *([FAKE] * 16), None),
          lib.mfvit_prenorm_xattn_forward(cfg, *([FAKE] * 5), None), lib.mfvit_prenorm_xattn_backward(cfg, *([FAKE] * 8), None),
          lib.mfvit_xattn_forward(cfg, *([FAKE] * 4), None), lib.mfvit_xattn_backward(cfg, *([FAKE] * 6), None)]
    if L == 1 and pm == 0:
        rc += [lib.mfvit_fusion_forward(cfg, *([FAKE] * 11), None), lib.mfvit_fusion_backward(cfg, *([FAKE] * 16), None)]
    return rc


@pytest.mark.parametrize("L,pm", [(1, 0), (2, 1)])
def test_class_and_token_ranges_are_checked_on_the_host(L, pm):
    from mfvit.fusion import fusion_cfg
    for C in (1, 64):
        assert all(q > 0 for q in _queries(fusion_cfg(3, 9, C), L, pm))
    for C in (0, 65, -1):
        cfg = fusion_cfg(3, 9, C)
        assert _queries(cfg, L, pm) == [0] * len(_queries(cfg, L, pm))
        assert set(_calls(cfg, L, pm)) == {EINVAL}
    for T in (0, 1, -5):
        cfg = fusion_cfg(2, T, 3)
        assert _queries(cfg, L, pm) == [0] * len(_queries(cfg, L, pm))
        assert set(_calls(cfg, L, pm)) == {EINVAL}
    assert all(q > 0 for q in _queries(fusion_cfg(2, 2, 3), L, pm))


@pytest.mark.parametrize("dim,heads,t_max", [(384, 3, 3200), (384, 6, 2596), (384, 12, 1220), (768, 3, 1280), (768, 6, 1280), (768, 12, 866)])
def test_token_limit_is_the_lds_of_the_streaming_passes(dim, heads, t_max):
    """The last accepted and the first refused token count per (dim, heads), as include/mfvit.h documents them: worked out from the launch
    code's LDS sizes (tests/fusion_edges_ref.py::T_MAX), not read back from the library."""
    from mfvit.fusion import fusion_cfg
    if (dim, heads) in fe.T_MAX:
        assert fe.T_MAX[(dim, heads)] == t_max
    for L, pm in ((1, 0), (2, 1)):
        assert all(q > 0 for q in _queries(fusion_cfg(1, t_max, 3, dim, heads), L, pm))
        for T in (t_max + 1, 2 * t_max, 1 << 30, (1 << 31) - 1):
            cfg = fusion_cfg(1, T, 3, dim, heads)
            assert _queries(cfg, L, pm) == [0] * len(_queries(cfg, L, pm))
            # (the calls themselves are made with real buffers: tests/test_fusion_edges_gpu.py::test_first_refused_token_count_launches_nothing)
    assert all(q > 0 for q in _queries(fusion_cfg(1, 577, 3, dim, heads), 1, 0))       # vit_base at 384 px is legal at every head count
