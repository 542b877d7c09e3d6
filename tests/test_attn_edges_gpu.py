"""GPU: the attention core (mfvit_attention_fwd / _bwd, and the dropout entries for one case) at the boundaries between its kernel families and
on peaked logits, against float64 - the cases, inputs, references and tolerances of tests/attn_edges_ref.py, whose CPU side is
tests/test_attn_edges_cpu.py.  Every test first asks mfvit_attention_plan which family the call takes and asserts that it is the one the case
names: a case chosen for one kernel cannot silently test another when a threshold moves.  Log: parity_attention_edges.txt, next to test_precision_gpu.py's.

The float64 references run on the GPU (plain torch matmul / exp in float64 on the rounded operands): the largest is 12 heads x 1121^2."""
import functools

import pytest
import torch

import attn_edges_ref as R
from mfvit import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 4096                      # bytes of 0xFF in front of, between and behind the carved outputs


def plan(mode_name, c, backward):
    return ops.attention_plan(R.CODE[mode_name], c.B, c.T, c.H, c.d, backward)["family"]


@functools.lru_cache(maxsize=1)
def gate_open():
    """2 x CUs lies between 504 and 516 pairs on this device (an MI355X has 256)."""
    return (ops.attention_plan(2, 42, 197, 12, 32)["family"], ops.attention_plan(2, 43, 197, 12, 32)["family"]) == ("pair", "fwd_pp")


def check_family(case, mode_name):
    if case.B > 2 and not gate_open():
        pytest.skip("2 x the compute units of this device does not lie between 504 and 516 pairs")
    named = R.named_families(case, mode_name)
    got = tuple(plan(mode_name, case, bw) if R.runs(case, mode_name, bw) else None for bw in (False, True))
    assert got == named, (case.name, mode_name, case.why)
    return got


@functools.lru_cache(maxsize=2)
def prepared(name, mode_name):
    """One case in one mode: the packed operands, the rounded ones in float64 on the GPU, the dropout mask, the forward reference.  Shared by the
    tests of the pair; nobody writes to it."""
    c, mode = R.BY_NAME[name], R.MODES[mode_name]
    qkv, dout = R.inputs(name)
    keep = ops.dropout_mask(c.drop, R.DROP_SEED, R.DROP_SITE, c.B * c.H * c.T * c.T).reshape(c.B, c.H, c.T, c.T) if c.drop else None
    p = dict(qkv=mode.pack_qkv(qkv), dout=mode.pack(dout), qr=mode.rounded_qkv(qkv).to(DEV), dr=mode.rounded(dout).to(DEV), keep=keep)
    p["o_ref"], p["l_ref"] = R.ref_fwd(p["qr"], c.H, keep, c.drop)
    return p


def run_fwd(c, mode, p):
    if c.drop:
        return ops.attention_drop_fwd(p["qkv"], c.H, c.drop, R.DROP_SEED, R.DROP_SITE, split=mode.split)
    return ops.attention_fwd(p["qkv"], c.H, split=mode.split)


def run_bwd(c, mode, p, out, lse, want_dbias):
    if c.drop:
        return ops.attention_drop_bwd(p["qkv"], out, p["dout"], lse, c.H, c.drop, R.DROP_SEED, R.DROP_SITE, split=mode.split), None
    return ops.attention_bwd(p["qkv"], out, p["dout"], lse, c.H, want_dbias=want_dbias, split=mode.split)


def unpack(mode, y):
    """Stored tensor -> float64 values on the GPU."""
    return ops.split_unpack(y).double() if mode.split else y.double()


def dbias_reorder_bound(dqkv_vals, M):
    """Two float-atomic column sums of the same M rows differ by their summation order only: each is within (chain length) x 2^-24 x sum |x| of
    the exact sum, the chain being the 64 rows of a workgroup and then one atomic per workgroup."""
    return 2.0 * (64 + M / 64.0) * 2.0 ** -24 * float(dqkv_vals.abs().sum((0, 1)).max())


# ---------------------------------------------------------------------------------------------------------------------------------- parity
def _parity(case, mode_name):
    mode = R.MODES[mode_name]
    fam = check_family(case, mode_name)
    p = prepared(case.name, mode_name)
    out, lse = run_fwd(case, mode, p)
    e_o, e_l = R.scale_err(unpack(mode, out), p["o_ref"]), R.scale_err(lse, p["l_ref"])
    line = f"{case.name}[{mode_name}] fwd {fam[0]} out {e_o:.2e} lse {e_l:.2e}"
    if fam[1] is None:                                                       # the forward alone is accepted (x3f16 beyond T = 224, fp32 beyond 620 / 315)
        R.log(line)
        assert e_o < mode.tol and e_l < R.LSE_TOL, line
        return
    g_ref, b_ref = R.ref_bwd(p["qr"], unpack(mode, out), lse, p["dr"], case.H, p["keep"], case.drop)
    dqkv, dbias = run_bwd(case, mode, p, out, lse, True)
    got = unpack(mode, dqkv)
    es = R.dqkv_errs(got, g_ref, case.B, case.T)
    e_b = 0.0 if dbias is None else R.scale_err(dbias, b_ref)
    line += f" | bwd {fam[1]} dq {es[0]:.2e} dk {es[1]:.2e} dv {es[2]:.2e} dbias {e_b:.2e}"
    R.log(line)
    t = R.bwd_tol(mode)
    assert e_o < mode.tol and e_l < R.LSE_TOL and max(es[0], es[2]) < t and es[1] < R.dk_bound(case, mode) and e_b < t, line
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(unpack(mode, out)).all())
    if dbias is not None:                                                    # want_dbias the other way: the same gradient bits, no sums
        dqkv2, none = run_bwd(case, mode, p, out, lse, False)
        assert none is None and torch.equal(dqkv2, dqkv), line


BOUNDARY_PAIRS = R.pairs(R.BOUNDARY)
PEAKED_PAIRS = R.pairs(R.PEAKED)


@pytest.mark.parametrize("case,mode_name", BOUNDARY_PAIRS, ids=R.pair_ids(BOUNDARY_PAIRS))
def test_parity_at_the_family_boundaries(case, mode_name):
    _parity(case, mode_name)


@pytest.mark.parametrize("case,mode_name", PEAKED_PAIRS, ids=R.pair_ids(PEAKED_PAIRS))
def test_parity_on_peaked_logits(case, mode_name):
    _parity(case, mode_name)


def test_every_family_ran_in_every_dtype_it_exists_for():
    """What the two parity tests above covered, from the plan of this device."""
    if not gate_open():
        pytest.skip("2 x the compute units of this device does not lie between 504 and 516 pairs")
    seen = {}
    for c, m in BOUNDARY_PAIRS + PEAKED_PAIRS:
        for bw in (False, True):
            if R.runs(c, m, bw):
                seen.setdefault(plan(m, c, bw), set()).add(m)
    sixteen = {"bf16x3", "fp16", "bf16", "x3f16"}
    assert seen == {"exact": {"fp32"}, "pair": sixteen, "fwd_pp": {"bf16x3", "x3f16"}, "bwd_padded": sixteen, "bwd_unpadded": {"fp16", "bf16"},
                    "bwd_sp": sixteen, "stream": {"bf16x3", "fp16", "bf16"}}


# ------------------------------------------------------------------------------------------- one case per family with T % 32 != 0, per mode
EDGE_NAMES = ("d32-T1", "d32-T2", "d32-T33", "d32-T129-B43", "d32-T193-B43", "d32-T225", "d32-T417", "d32-T449", "d32-T577", "d32-T1121",
              "d64-T65", "d96-T65", "peak-pp197-stairs-21", "peak-T225-stairs-21")
EDGE_PAIRS = R.pairs([R.BY_NAME[n] for n in EDGE_NAMES], backward=True)


def carve(sizes):
    """One uint8 buffer of 0xFF bytes (a NaN in bf16, fp16 and f32 alike); returns it and the byte range of every carved tensor, 256-byte
    aligned, with BAND bytes in front of, between and behind them."""
    offs, n = [], BAND
    for s in sizes:
        offs.append((n, n + s))
        n = (n + s + BAND + 255) // 256 * 256
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV), offs


def bands_untouched(buf, offs):
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for a, b in offs:
        mask[a:b] = False
    return bool((buf[mask] == 0xFF).all())


def out_dtype(mode):
    return torch.float32 if mode.name == "fp32" else (torch.bfloat16 if mode.name in ("bf16", "bf16x3", "x3f16") else torch.float16)


def raw_call(c, mode, qkv, dout, buf, offs, want_bwd=True):
    """mfvit_attention_fwd (and _bwd) through the raw ABI into tensors carved from buf: (rc_fwd, rc_bwd, out, lse, dqkv)."""
    e, dt = (2 if mode.split else 1), out_dtype(mode)
    D = c.H * c.d
    out = buf[offs[0][0]:offs[0][1]].view(dt).view(c.B, c.T, D * e)
    lse = buf[offs[1][0]:offs[1][1]].view(torch.float32).view(c.B, c.H, c.T)
    dqkv = buf[offs[2][0]:offs[2][1]].view(dt).view(c.B, c.T, 3 * D * e)
    L, code = _lib.lib(), R.CODE[mode.name]
    rc_f = L.mfvit_attention_fwd(code, qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), c.B, c.T, c.H, c.d, _lib.stream())
    rc_b = None
    if want_bwd:
        rc_b = L.mfvit_attention_bwd(code, qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), None, c.B, c.T, c.H, c.d,
                                     _lib.stream())
    torch.cuda.synchronize()
    return rc_f, rc_b, out, lse, dqkv


def carve_sizes(c, mode):
    esz = (4 if mode.name == "fp32" else 2) * (2 if mode.split else 1)
    D = c.H * c.d
    return [c.B * c.T * D * esz, c.B * c.H * c.T * 4, c.B * c.T * 3 * D * esz]


@pytest.mark.parametrize("case,mode_name", EDGE_PAIRS, ids=R.pair_ids(EDGE_PAIRS))
def test_every_entry_is_written_and_nothing_beyond(case, mode_name):
    """out, lse and dqkv carved out of one NaN-filled buffer with NaN bands around them: all of every output comes back finite (rows of the last,
    partial tile included), and not a byte of a band has changed."""
    mode = R.MODES[mode_name]
    check_family(case, mode_name)
    qkv, dout = R.inputs(case.name)
    buf, offs = carve(carve_sizes(case, mode))
    rc_f, rc_b, out, lse, dqkv = raw_call(case, mode, mode.pack_qkv(qkv), mode.pack(dout), buf, offs)
    assert rc_f == 0 and rc_b == 0
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dqkv.float()).all())
    assert bands_untouched(buf, offs)


@pytest.mark.parametrize("case,mode_name", EDGE_PAIRS, ids=R.pair_ids(EDGE_PAIRS))
def test_repeat_runs_give_the_same_bits(case, mode_name):
    """out, lse and dqkv: the same bits from two runs in every family.  dbias is summed by float atomics: rounding-level agreement only."""
    mode = R.MODES[mode_name]
    check_family(case, mode_name)
    qkv, dout = R.inputs(case.name)
    q, d = mode.pack_qkv(qkv), mode.pack(dout)
    runs = []
    for _ in range(2):
        out, lse = ops.attention_fwd(q, case.H, split=mode.split)
        dqkv, dbias = ops.attention_bwd(q, out, d, lse, case.H, split=mode.split)
        runs.append((out, lse, dqkv, dbias))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a, b)
    bound = dbias_reorder_bound(unpack(mode, runs[0][2]), case.B * case.T)
    assert float((runs[0][3] - runs[1][3]).abs().max()) <= bound


# -------------------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("ref", R.REFUSALS, ids=[f"{r[0]}-T{r[2]}-d{r[4]}-{'bwd' if r[5] else 'fwd'}" for r in R.REFUSALS])
def test_refused_calls_leave_the_outputs_untouched(ref):
    m, B, T, H, d, backward, code = ref
    mode = R.MODES[m]
    c = R.Case("refused", B, T, H, d, (m,), None, None, "")
    qkv = mode.pack_qkv(torch.zeros(B, T, 3 * H * d))
    dout = mode.pack(torch.zeros(B, T, H * d))
    buf, offs = carve(carve_sizes(c, mode))
    if backward:                                                             # out and lse are inputs here: the NaN bytes as they are
        at = [buf[a:b].data_ptr() for a, b in offs]
        rc = _lib.lib().mfvit_attention_bwd(R.CODE[m], qkv.data_ptr(), at[0], dout.data_ptr(), at[1], at[2], None, B, T, H, d, _lib.stream())
    else:
        rc = raw_call(c, mode, qkv, dout, buf, offs, want_bwd=False)[0]
    torch.cuda.synchronize()
    assert rc == code and bool((buf == 0xFF).all())


# --------------------------------------------------------------------------------------------------------------------- sample independence
@pytest.mark.parametrize("name,mode_name", [("peak-T448-stairs-21", "bf16"), ("peak-T225-stairs-21", "bf16x3")])
def test_sample_zero_does_not_depend_on_the_batch(name, mode_name):
    """Sample 0 of B = 2 equals the B = 1 run bit for bit (unpadded two-phase backward; per-pair forward with the streaming backward)."""
    case, mode = R.BY_NAME[name], R.MODES[mode_name]
    assert case.B == 2
    check_family(case, mode_name)
    assert check_family(case._replace(B=1), mode_name) == R.named_families(case, mode_name)
    qkv, dout = R.inputs(name)
    res = []
    for n in (2, 1):
        q, d = mode.pack_qkv(qkv[:n]), mode.pack(dout[:n])
        out, lse = ops.attention_fwd(q, case.H, split=mode.split)
        dqkv, _ = ops.attention_bwd(q, out, d, lse, case.H, want_dbias=False, split=mode.split)
        res.append((out[:1], lse[:1], dqkv[:1]))
    for a, b in zip(*res):
        assert torch.equal(a, b)
