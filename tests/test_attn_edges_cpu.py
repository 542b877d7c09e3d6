"""CPU: what the attention edge tests (tests/test_attn_edges_gpu.py) stand on.
  * the launchers' plan (mfvit_attention_plan: host only) reports, for every case, the family, the row tiles and the LDS bytes that the case names
    (by hand) and that the launchers' formulas give (attn_edges_ref.expect) - three statements of one decision;
  * the refusals;
  * the float64 references equal torch autograd in float64;
  * every peaked case takes the lazy rescales it declares, at both thresholds, and no other row takes any;
  * a float64 emulation of the lazy-maximum forward meets the project's tolerances on every peaked case, misses them as soon as a rescale is
    left out - and every such mutant passes on randn inputs of the same shape: the gap the peaked cases close."""
import pytest
import torch

import attn_edges_ref as R
from mfvit import _lib, ops


def device_cus():
    """attention_mfma.hip::attn_cus: the current device's CUs rounded down to 8; 256 without a device."""
    if torch.cuda.is_available():
        return max(8, torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count & ~7)
    return 256


def plan(mode_name, c, backward):
    return ops.attention_plan(R.CODE[mode_name], c.B, c.T, c.H, c.d, backward)


def plan_code(mode_name, B, T, H, d, backward):
    out = (_lib.ctypes.c_int32 * 6)(*([-7] * 6))
    rc = _lib.lib().mfvit_attention_plan(R.CODE[mode_name], B, T, H, d, int(backward), out)
    return rc, list(out)


@pytest.fixture(autouse=True)
def default_switch(monkeypatch):
    monkeypatch.delenv("MFVIT_ATTN_BWD_SP", raising=False)


# ------------------------------------------------------------------------------------------------------------------------------- plan pins
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_plan_reports_the_family_each_case_names(case):
    cus = device_cus()
    gate_open = 504 < 2 * cus <= 516
    for m in case.modes:
        named = R.named_families(case, m)
        for bw in (False, True):
            want = R.expect(m, case.B, case.T, case.H, case.d, bw, cus=cus)
            if isinstance(want, int):
                rc, out = plan_code(m, case.B, case.T, case.H, case.d, bw)
                assert rc == want and out == [-7] * 6, (case.name, m, bw)
                assert named[bw] is None or m == "x3f16", (case.name, m, bw)
                continue
            got = plan(m, case, bw)
            assert got == want, (case.name, m, bw)
            if gate_open or case.B <= 2:
                assert got["family"] == named[bw], (case.name, m, bw, case.why)
            assert got["lds"] <= R.LDS_LIMIT and got["tiles"] == (0 if m == "fp32" else (case.T + 31) // 32)


def test_pinned_numbers_of_the_families():
    """A handful of plans as plain numbers, worked out from the kernels' LDS layouts by hand (256 CUs)."""
    if device_cus() != 256:
        pytest.skip("the pins are for 256 compute units")
    P = ops.attention_plan
    # per-pair forward: Tpad x (padded K row + V row): 224 x (80 + 64), split 224 x (144 + 128)
    assert P(1, 2, 197, 12, 32) == dict(family="pair", tiles=7, lds=32256, grid=24, threads=256, lds2=0)
    assert P(2, 2, 197, 12, 32)["lds"] == 60928
    # persistent forward, T = 197: two slots of K + V images of 200 rows x 128 B, 24 overrun rows, 7 staging tiles of 32 x 144 B
    assert P(4, 43, 197, 12, 32) == dict(family="fwd_pp", tiles=7, lds=4 * 200 * 128 + 24 * 128 + 7 * 32 * 144, grid=256, threads=512, lds2=0)
    # two-phase backward: four images + lse / D rows + the next pair's O rows; padded 80-B pitch up to Tpad 416, 64-B above
    assert P(1, 1, 416, 12, 32, True) == dict(family="bwd_padded", tiles=13, lds=416 * (4 * 80 + 8 + 64), grid=12, threads=512, lds2=0)
    assert P(3, 1, 417, 12, 32, True) == dict(family="bwd_unpadded", tiles=14, lds=448 * (4 * 64 + 8 + 64), grid=12, threads=512, lds2=0)
    assert P(1, 1, 480, 12, 32, True)["lds"] == 480 * 328 and P(1, 1, 481, 12, 32, True)["family"] == "stream"
    # single-pass backward: four images of 208 (plain: 16-row pieces) / 200 rows, 14 dS tiles of 32 rows, the row constants, 32 B of maxima
    assert P(1, 43, 197, 12, 32, True) == dict(family="bwd_sp", tiles=7, lds=4 * 208 * 64 + 14 * 32 * 64 + 2 * 224 * 4 + 32, grid=256, threads=512, lds2=0)
    assert P(2, 43, 200, 12, 32, True)["family"] == "bwd_sp" and P(2, 43, 201, 12, 32, True)["family"] == "bwd_padded"   # split: 208-row images: 165,664 B
    # streaming: two 64-row chunks at pitch 2 d (x 2 split) + 16; the dK / dV launch adds the chunk's lse and D rows
    assert P(2, 1, 577, 12, 32, True) == dict(family="stream", tiles=19, lds=128 * 144, grid=12 * 5, threads=256, lds2=128 * 144 + 512)
    assert P(3, 2, 129, 4, 96) == dict(family="stream", tiles=5, lds=128 * 208, grid=16, threads=256, lds2=0)
    # exact: K and V as f32, backward + two rows of T floats
    assert P(0, 2, 33, 12, 32, True) == dict(family="exact", tiles=0, lds=2 * 33 * 32 * 4 + 2 * 33 * 4, grid=24, threads=256, lds2=0)


def test_every_family_is_taken_by_a_case_in_every_dtype_it_exists_for():
    seen = {}
    for c, m in R.pairs(R.CASES):
        for bw in (False, True):
            e = R.expect(m, c.B, c.T, c.H, c.d, bw)
            if not isinstance(e, int):
                seen.setdefault(e["family"], set()).add(m)
    sixteen = {"bf16x3", "fp16", "bf16", "x3f16"}
    assert seen == {"exact": {"fp32"}, "pair": sixteen, "fwd_pp": {"bf16x3", "x3f16"}, "bwd_padded": sixteen, "bwd_unpadded": {"fp16", "bf16"},
                    "bwd_sp": sixteen, "stream": {"bf16x3", "fp16", "bf16"}}


def test_qkv_dtype_flips_at_224():
    for T in (1, 197, 224):
        assert ops.attention_qkv_dtype(2, T, 32) == 4 == R.qkv_code("bf16x3", T, 32)
    for T, d in ((225, 32), (577, 32), (197, 64), (129, 96)):
        assert ops.attention_qkv_dtype(2, T, d) == 2 == R.qkv_code("bf16x3", T, d)
    for code in (0, 1, 3):
        assert ops.attention_qkv_dtype(code, 197, 32) == code


def test_the_backward_switch_is_honoured(monkeypatch):
    if device_cus() != 256:
        pytest.skip("516 pairs stand above the gate of 256 compute units")
    assert ops.attention_plan(1, 43, 197, 12, 32, True)["family"] == "bwd_sp"
    monkeypatch.setenv("MFVIT_ATTN_BWD_SP", "0")            # (tests/conftest.py: MFVIT_AB_LIVE=1, switches are read at every call)
    got = ops.attention_plan(1, 43, 197, 12, 32, True)
    assert got == R.expect("bf16", 43, 197, 12, 32, True, bwd_sp=False) and got["family"] == "bwd_padded"


# -------------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    for m, B, T, H, d, bw, code in R.REFUSALS:
        rc, out = plan_code(m, B, T, H, d, bw)
        assert rc == code == R.expect(m, B, T, H, d, bw) and out == [-7] * 6, (m, T, d, bw)
    # the last accepted neighbours
    for m, T, H, d, bw in (("x3f16", 224, 12, 32, True), ("x3f16", 576, 12, 32, False), ("fp32", 620, 12, 32, True), ("fp32", 621, 12, 32, False), ("fp32", 640, 12, 32, False),
                           ("fp32", 315, 6, 64, True), ("fp32", 320, 6, 64, False)):
        assert plan_code(m, 1, T, H, d, bw)[0] == 0, (m, T, d, bw)
    # arguments outside the domain, and a NULL plan
    for B, T, H in ((0, 197, 12), (2, 0, 12), (2, 197, 0)):
        assert plan_code("bf16", B, T, H, 32, False)[0] == R.EINVAL
    assert _lib.lib().mfvit_attention_plan(1, 2, 197, 12, 32, 0, None) == R.EINVAL
    assert plan_code("bf16", 2, 197, 3, 128, False)[0] == R.EINVAL and _lib.lib().mfvit_attention_plan(9, 2, 197, 12, 32, 0, (_lib.ctypes.c_int32 * 6)()) == R.EINVAL


# ------------------------------------------------------------------------------------------------------------------------ reference checks
@pytest.mark.parametrize("name", ["d32-T33", "d64-T65", "d96-T65", "d32-T1", "peak-pair197-stairs-21", "peak-d96-T129-stairs-21-drop"])
def test_references_equal_float64_autograd(name):
    c = R.BY_NAME[name]
    qkv, dout = (x.double() for x in R.inputs(name))
    keep = None
    if c.drop:
        keep = torch.rand(c.B, c.H, c.T, c.T, generator=torch.Generator().manual_seed(3)) >= c.drop
    qd = qkv.clone().requires_grad_(True)
    q, k, v = R.heads(qd, c.H, 3)
    s = (q @ k.transpose(-1, -2)) * c.d ** -0.5
    att = s.softmax(-1)
    if keep is not None:
        att = att * keep.double() / (1 - c.drop)
    o_auto = R.merge(att @ v)
    o_auto.backward(dout)
    out, lse = R.ref_fwd(qkv, c.H, keep, c.drop)
    dqkv, dbias = R.ref_bwd(qkv, out, lse, dout, c.H, keep, c.drop)
    assert R.scale_err(out, o_auto.detach()) < 1e-13 and R.scale_err(lse, torch.logsumexp(s.detach(), -1)) < 1e-14
    assert R.scale_err(dqkv, qd.grad) < 1e-12 and R.scale_err(dbias, qd.grad.sum((0, 1))) < 1e-12
    if c.T == 1:
        g = dqkv.view(c.B, 1, 3, -1)
        # (one key: P = 1 and dP = D up to the order of two float64 dot products)
        assert float(g[:, :, :2].abs().max()) < 1e-13 * float(g[:, :, 2].abs().max())


# ------------------------------------------------------------------------------------------------------------------------- crossing counts
@pytest.mark.parametrize("case", R.PEAKED, ids=[c.name for c in R.PEAKED])
def test_peaked_cases_take_the_rescales_they_declare(case):
    qkv, _ = R.inputs(case.name)
    a, _ = R.peak_profile(case)
    up = a > 0
    assert int(up.sum()) >= 30 and not bool(up[:32].any())
    for m in ("x3f16", "bf16x3"):
        s = R.logits(R.MODES[m].rounded_qkv(qkv), case.H)
        for thr_log2, want in zip((14.0, 24.0), case.cross):
            n = R.lazy_crossings(s, thr_log2 * R.LN2)
            if want is None:                                   # not declared (attn_edges_ref.py): most rows cross once, none twice
                assert float((n[..., up] == 1).double().mean()) > 0.99 and int(n.max()) == 1 and int(n[..., ~up].max()) == 0
                continue
            assert bool((n[..., up] == want).all()), (case.name, m, thr_log2, n[..., up].unique(return_counts=True))
            assert int(n[..., ~up].max()) == 0, (case.name, m, thr_log2)
    assert float(s.max()) < 50.0                                       # two stairs of 21 and the noise's maximum
    s0 = R.logits(R.MODES["x3f16"].rounded_qkv(R.randn_twin(case)), case.H)
    assert int(R.lazy_crossings(s0, 14.0 * R.LN2).max()) == 0          # randn: not one rescale behind tile 0, at either threshold


# -------------------------------------------------------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("case", R.PEAKED, ids=[c.name for c in R.PEAKED])
def test_a_forward_without_its_rescale_is_caught_on_peaked_inputs_only(case):
    """The honest emulation on the whole case; the mutants on its first two samples (their inputs do not depend on the batch size)."""
    qkv_all, _ = R.inputs(case.name)
    for m, want in zip(("x3f16", "bf16x3"), case.cross):
        mode = R.MODES[m]
        qr = mode.rounded_qkv(qkv_all)
        o_ref, l_ref = R.ref_fwd(qr, case.H)
        assert R.meets(*R.emulate_lazy(qr, case.H, m), o_ref, l_ref, mode.tol), (case.name, m)
        qr, o_ref, l_ref = qr[:2], o_ref[:2], l_ref[:2]
        if want is None:
            continue
        for mutant in ("skip_o", "skip_lsum"):
            ok = R.meets(*R.emulate_lazy(qr, case.H, m, mutant), o_ref, l_ref, mode.tol)
            assert ok == (want == 0), (case.name, m, mutant)
        if m == "x3f16":
            # never rescaling: P leaves fp16's range (inf) or the sums lose the row - unless nothing crosses.  (Split bf16 keeps f32's exponent
            # range in P, o and lsum: there the threshold guards nothing below a gap of 2^127 and a forward that never fires stays correct.)
            ok = R.meets(*R.emulate_lazy(qr, case.H, m, "never"), o_ref, l_ref, mode.tol)
            assert ok == (want == 0), (case.name, m, "never")
        q0 = mode.rounded_qkv(R.randn_twin(case)[:2])
        o0, l0 = R.ref_fwd(q0, case.H)
        for mutant in (None, "skip_o", "skip_lsum", "never"):
            assert R.meets(*R.emulate_lazy(q0, case.H, m, mutant), o0, l0, mode.tol), (case.name, m, mutant, "randn")


# ------------------------------------------------------------------------------------------ the format model behind the two widened bounds
@pytest.mark.parametrize("key", sorted(R.MODEL_BOUNDS), ids=[k[0] for k in sorted(R.MODEL_BOUNDS)])
def test_the_split_bf16_format_alone_explains_the_widened_dk_bounds(key):
    """attn_edges_ref.MODEL_BOUNDS: the recorded model error is what the model gives, it exceeds the project's bound by itself, the kernel's
    measured error lies within 2 % of it, and everything else of the model stays inside the project's tolerances."""
    case, mode = R.BY_NAME[key[0]], R.MODES[key[1]]
    rec = R.MODEL_BOUNDS[key]
    e_o, e_l, (e_q, e_k, e_v) = R.model_bf16x3(*R.inputs(case.name), case.H)
    assert abs(e_k - rec["model"]) < 0.01 * rec["model"], e_k
    assert e_k > R.bwd_tol(mode) and abs(rec["measured"] - rec["model"]) < 0.02 * rec["model"] and rec["measured"] < R.dk_bound(case, mode)
    assert e_o < mode.tol and e_l < R.LSE_TOL and max(e_q, e_v) < R.bwd_tol(mode)
    # the same model on a jump of 13 (the largest product 77, once): inside the bound, like the kernels
    other = R.BY_NAME["peak-pair197-jump3-13"]
    assert max(R.model_bf16x3(*R.inputs(other.name), other.H)[2]) < R.bwd_tol(mode)
