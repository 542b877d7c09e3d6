"""CPU: what the weight-gradient edge tests (tests/test_wgrad_edges_gpu.py) stand on.
  * the launchers' split plan (mfvit_linear_wgrad_plan: host only) reports, for every directed case of the GPU file, the kernel, the splits, the
    rows of the last split and the use of the scratch / the bias partials the case was chosen for - pinned numbers (tests/wgrad_ref.py);
  * the float64 reference equals torch's float64 matmul / sum, plain and remapped;
  * the exact inputs fulfil the exactness condition, and an f32 summation in a shuffled order equals the reference bit for bit;
  * the exact comparison flags every seeded mistake of the list in `MUTATIONS`;
  * the Gaussian gate holds for an honest f32 summation and flags a documented share of the elements when the last row is dropped."""
import pytest
import torch

import wgrad_ref as R
from mfvit import _lib, ops

SCRATCH_TILES = 384            # include/mfvit.h: MFVIT_WGRAD_SCRATCH_FLOATS / (128 * 128)


def plan(kind, M, N=128, K=128, **kw):
    return ops.linear_wgrad_plan(R.CODE[kind], M, N, K, **kw)


@pytest.fixture(autouse=True)
def whole_chip(monkeypatch):
    monkeypatch.delenv("MFVIT_TN_GLDS", raising=False)
    _lib.lib().mfvit_set_stream_share(1)
    yield
    _lib.lib().mfvit_set_stream_share(1)


# ------------------------------------------------------------------------------------------------------------------------------- plan pins
@pytest.mark.parametrize("kind", ["split", "bf16", "fp16"])
def test_plan_lds_dma_last_split(kind):
    for r in R.GLDS_R[kind]:
        pin = R.glds_pin(kind, r)
        M = R.GLDS_M0 + r
        R.check_plan(plan(kind, M), pin, False, False)
        R.check_plan(plan(kind, M, bias=True), pin, False, False)
        R.check_plan(plan(kind, M, scratch=True), pin, True, False)
        R.check_plan(plan(kind, M, scratch=True, bias=True), pin, True, True)
        R.check_plan(plan(kind, M, scratch=True, bias=True, bias_aligned=False), pin, True, False)      # float atomics onto dbias
        R.check_plan(plan(kind, M, scratch=True, lddw=132), pin, True, False)                            # guard columns: a pitch of K + 4 keeps the scratch
        kr, st0, valid = pin["kr"], *R.last_stage(plan(kind, M))
        assert st0 + valid == M and 1 <= valid <= kr
    # the hint of a second kernel stream halves the target (128 workgroups): one tile still gets every split its rows allow
    _lib.lib().mfvit_set_stream_share(2)
    for r in (1, 33):
        R.check_plan(plan(kind, R.GLDS_M0 + r, scratch=True, bias=True), R.glds_pin(kind, r), True, True)


@pytest.mark.parametrize("kind", ["split", "bf16", "fp16"])
def test_plan_lds_dma_pair_one_split_remap(kind):
    kr = R.GLDS_KR[kind]
    for r in (1, kr - 1, kr + 1):
        for na, nb in ((128, 128), (384, 128)):
            pin = R.glds_pin(kind, r, tiles=(na + nb) // 128)
            R.check_plan(plan(kind, R.GLDS_M0 + r, na, 128, N2=nb, bias=True), pin, False, False)    # (the paired C entry passes no scratch)
    with pytest.raises(_lib.MfvitError, match="-38"):
        plan(kind, 2047, 128, 128, N2=128)
    # 144 tiles: more than half the target, one split, the scratch is not used
    for M in (2048, 2053):
        one = dict(kernel="glds", kr=kr, splits=1, chunk=-(-M // kr) * kr, last_rows=M, tiles=144)
        R.check_plan(plan(kind, M, 1536, 1536, scratch=True), one, False, False)
        R.check_plan(plan(kind, M, 1536, 1536, scratch=True, bias=True), one, False, False)
    for r in (1, 33):
        if kind == "split":
            R.check_plan(plan(kind, R.GLDS_M0 + r, remap=True, scratch=True), R.glds_pin(kind, r), True, False)
            R.check_plan(plan(kind, R.GLDS_M0 + r, remap=True, scratch=True, bias=True), R.tile_pin(kind, 2049) if r == 1 else
                         dict(kernel="tile", kr=64, splits=9, chunk=256, last_rows=33, tiles=4), True, True)     # remap + bias sums: gemm_tn_kernel
        else:
            assert plan(kind, R.GLDS_M0 + r, remap=True)["kernel"] == "tile"


@pytest.mark.parametrize("kind", R.KINDS)
def test_plan_tile_kernel(kind, monkeypatch):
    for M in R.tile_ms(kind):
        pin = R.tile_pin(kind, M)
        multi = pin["splits"] > 1
        R.check_plan(plan(kind, M, bias=True), pin, False, False)
        R.check_plan(plan(kind, M, bias=True, scratch=True), pin, multi, multi)
        R.check_plan(plan(kind, M, bias=True, bias_aligned=False, scratch=True), pin, multi, False)
        R.check_plan(plan(kind, M, bias=True, scratch=True, lddw=132), pin, multi, multi)
        if kind != "f32" or M > 512:
            R.check_plan(plan(kind, M, scratch=True), pin, multi, False)
        else:
            assert plan(kind, M, scratch=True)["kernel"] == "small"        # f32 up to 512 rows without bias sums / remap: gemm_small.hip
        if M in (R.TILE_KR[kind] + 1, 600):
            R.check_plan(plan(kind, M, remap=True, scratch=True, bias=True), pin, multi, multi)
            R.check_plan(plan(kind, M, remap=True), pin, False, False)
    if kind == "split":
        for M in R.tile_ms(kind):                                          # the narrowest split-bf16 shape: one 128 x 128 STORAGE tile
            pin = R.tile_pin(kind, M, n=64)
            R.check_plan(plan(kind, M, 64, 64, bias=True, scratch=True), pin, pin["splits"] > 1, pin["splits"] > 1)
    if kind == "f32":
        # tiles x splits == 384: the tile partials fit the scratch, the bias partials behind them (+ 2) do not
        p = plan(kind, 3072, 512, 512, bias=True, scratch=True)
        R.check_plan(p, dict(kernel="tile", kr=32, splits=24, chunk=128, last_rows=128, tiles=16), True, False)
        assert p["tiles"] * p["splits"] == SCRATCH_TILES
        assert plan(kind, 37) == dict(kernel="small", kr=0, splits=1, chunk=37, last_rows=37, scratch=False, kpart=False, tiles=0)
    else:
        monkeypatch.setenv("MFVIT_TN_GLDS", "0")
        for r in (1, 65):
            R.check_plan(plan(kind, R.GLDS_M0 + r, bias=True, scratch=True), R.tile_pin(kind, R.GLDS_M0 + r), True, True)
        monkeypatch.delenv("MFVIT_TN_GLDS")
        assert plan(kind, R.GLDS_M0 + 1)["kernel"] == "glds"


def test_plan_refusals():
    for kind, kw in (("bf16", dict(N=64)), ("split", dict(N=32)), ("f32", dict(K=96)), ("bf16", dict(M=0)), ("f32", dict(M=-3)),
                     ("bf16", dict(lddy=132)), ("split", dict(ldx=260)), ("f32", dict(lddy=130, bias=True)), ("fp16", dict(M=4096, ldx=132))):
        args = dict(M=600, N=128, K=128)
        args.update(kw)
        with pytest.raises(_lib.MfvitError, match="-22"):
            plan(kind, **args)
    assert _lib.lib().mfvit_linear_wgrad_plan(1, 600, 128, 128, 0, 128, 128, 128, 0, 0, 0, 16, (_lib.ctypes.c_int32 * 8)()) == -22      # unknown flag
    assert _lib.lib().mfvit_linear_wgrad_plan(1, 600, 128, 128, 0, 128, 128, 128, 0, 0, 0, 0, None) == -22


# ------------------------------------------------------------------------------------------------------------------------- reference pins
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("remap", [None, (7, 8, 1)])
def test_reference_is_float64_matmul(kind, remap):
    M, N, K = 211, 64, 96
    g = R.gen(3)
    rows = M if remap is None else R.remap_total(M, remap)
    dy, x = R.gauss_operand(g, (rows, N), 0.1), R.gauss_operand(g, (M, K), 1.0)
    idx = R.remap_rows(M, remap)
    if remap is not None:
        assert idx[:9].tolist() == [1, 2, 3, 4, 5, 6, 7, 9, 10] and rows == int(idx[-1]) + 1
        skipped = torch.ones(rows, dtype=torch.bool)
        skipped[idx] = False
        assert int(skipped.sum()) == rows - M
        dy[skipped] = float("nan")                                                     # never read
    ref = R.reference(dy, x, kind, remap=remap)
    if kind == "split":
        a, xx = dy[idx].double(), x.double()
        ah, xh = dy[idx].bfloat16().double(), x.bfloat16().double()
        al, xl = (dy[idx] - ah.float()).bfloat16().double(), (x - xh.float()).bfloat16().double()
        want = (ah + al).T @ (xh + xl) - al.T @ xl                                     # everything but lo*lo
        torch.testing.assert_close(ref["dw"], want, rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(ref["db"], (ah + al).sum(0), rtol=1e-13, atol=0)
        assert float((ref["dw"] - a.T @ xx).abs().max()) < 2.0 ** -15 * float(ref["absw"].max())    # hi + lo carries 16 bits of the value
        assert torch.equal(ops.split_unpack(R.pack(dy[idx], kind)).double(), ah + al)
        assert torch.equal(R.pack(x, kind), ops.split_pack(x))
    else:
        a, xx = dy[idx].to(R.TDTYPE[kind]).double(), x.to(R.TDTYPE[kind]).double()
        assert torch.equal(ref["dw"], a.T @ xx) and torch.equal(ref["db"], a.sum(0))
        assert torch.equal(ref["absw"], a.abs().T @ xx.abs()) and torch.equal(ref["absb"], a.abs().sum(0))
    assert bool(torch.isfinite(ref["dw"]).all()) and bool((ref["absw"] >= ref["dw"].abs()).all())


# ------------------------------------------------------------------------------------------------------------------------ exactness condition
def exact_cases():
    """(kind, M, N, K, remap, seed) of every exact case of the GPU file"""
    out = []
    for kind in ("split", "bf16", "fp16"):
        out += [(kind, R.GLDS_M0 + r, 128, 128, None, 0) for r in R.GLDS_R[kind]]
        out += [(kind, R.GLDS_M0 + r, n, 128, None, s) for r in (1, R.GLDS_KR[kind] - 1, R.GLDS_KR[kind] + 1) for n, s in ((384, 0), (128, 1))]
        out += [(kind, R.GLDS_M0 + 65, 128, 128, None, 0)]
    out += [("split", R.GLDS_M0 + r, 128, 128, (7, 8, 1), 0) for r in (1, 33)]
    for kind in R.KINDS:
        out += [(kind, M, 128, 128, None, 0) for M in R.tile_ms(kind)]
        out += [(kind, M, 128, 128, (7, 8, 1), 0) for M in (R.TILE_KR[kind] + 1, 600)]
    out += [("split", M, 64, 64, None, 0) for M in R.tile_ms("split")]
    out += [("f32", 37, 128, 128, None, 0)]
    return out


def test_exact_inputs_fulfil_the_condition():
    worst = {}
    for kind, M, N, K, remap, seed in exact_cases():
        dy, x, ref = R.exact_pair(kind, M, N, K, seed=seed, remap=remap)          # (asserts the condition, the pre-filled output included)
        worst[kind] = max(worst.get(kind, 0), ref["bound"])
        assert torch.equal(ref["dw"].float().double(), ref["dw"]) and torch.equal(ref["db"].float().double(), ref["db"])
        if kind == "split":                                                            # both parts carry data, hi is the integer
            ah, al = R.parts(dy[R.remap_rows(M, remap)], kind)
            assert torch.equal(ah, ah.round()) and float(al.abs().max()) == 3 / 1024 and float(ah.abs().max()) == 3
    assert worst["split"] < 2 ** 13 and worst["f32"] < 2 ** 16                         # (far inside 2^14 / 2^24)
    # the two large shapes.  512 x 512 at M = 3,072: the bound from the grid's largest value, no matmul needed.  N = K = 1,536: the abs-sum in f32 (a sum of
    # non-negative terms: within M 2^-24 of the true one, so a margin of 2^-10 decides), the float64 reference itself is left to the GPU file
    assert 3072 * 16 + 8 < R.exact_limit("f32")
    for kind in ("split", "bf16"):
        for M in (2048, 2053):
            dy, x = R.exact_operands(kind, M, 1536, 1536)
            absw, absb = R.abs_sums(dy, x, kind, dtype=torch.float32)
            assert float(absw.max()) + 8 < R.exact_limit(kind) * (1 - 2.0 ** -10) and float(absb.max()) + 8 < R.exact_limit(kind) * (1 - 2.0 ** -10)


@pytest.mark.parametrize("kind", R.KINDS)
def test_exact_inputs_are_order_independent_in_f32(kind):
    M = 2303
    dy, x, ref = R.exact_pair(kind, M, 128, 128)
    bound = ref["bound"]
    assert bound < (5000 if kind == "split" else 14000)                                # (measured 4,143 of 16,384 / 12,271 of 2^24 when the grids were chosen)
    for seed in range(3):
        assert torch.equal(R.f32_shuffled(dy, x, kind, seed=seed).double(), ref["dw"])
    if kind != "split":
        f = dy.float().T @ x.float()
        assert torch.equal(f.double(), ref["dw"])


# -------------------------------------------------------------------------------------------------------------------------------- mutations
def rows_except(M, lo, hi):
    return torch.cat([torch.arange(0, lo), torch.arange(hi, M)])


def mutants(kind, M, remap=None):
    """name -> (dw, db) with one mistake each, computed on the exact inputs of (kind, M) under the launcher's plan"""
    dy, x, _ = R.exact_pair(kind, M, 128, 128, remap=remap)
    p = plan(kind, M, scratch=True, bias=True, remap=remap is not None)
    ref = lambda **kw: R.reference(dy, x, kind, remap=remap, **kw)
    good = ref()
    out = {}
    r = ref(rows=torch.arange(M - 1))
    out["last row dropped"] = (r["dw"], r["db"])
    st0, valid = R.last_stage(p)
    r = ref(rows=torch.arange(st0))
    out["last stage of the last split dropped"] = (r["dw"], r["db"])
    s = p["splits"] // 2
    r = ref(rows=torch.arange(s * p["chunk"], min(M, (s + 1) * p["chunk"])))
    out["one split counted twice"] = (good["dw"] + r["dw"], good["db"] + r["db"])
    if kind == "split":
        r = ref(drop_lohi=True)
        out["lo*hi term dropped"] = (r["dw"], good["db"])
    if p["splits"] > 1:
        extra = max(1, p["kr"] - valid)                                                # split 0 runs on into the first rows of split 1
        r = ref(rows=torch.arange(p["chunk"], p["chunk"] + extra))
        out["rows past a split's end taken from the next split"] = (good["dw"] + r["dw"], good["db"] + r["db"])
    if valid < p["kr"]:
        r = ref(rows=torch.tensor([M - 1]))                                            # the clamped re-fetch of row M - 1, not zeroed
        out["clamped rows past the end not zeroed"] = (good["dw"] + (p["kr"] - valid) * r["dw"], good["db"] + (p["kr"] - valid) * r["db"])
    out["bias from the other 32-row block"] = (good["dw"], good["db"].reshape(-1, 2, 32).flip(1).reshape(-1))
    if remap is not None:
        shifted = (remap[0], remap[1], remap[2] - 1)
        ok = dy.clone()
        ok[torch.isnan(ok)] = 1.0                                                      # (the skipped rows: what a wrong offset reads)
        r = R.reference(ok, x, kind, remap=shifted)
        out["remap off by row_off"] = (r["dw"], r["db"])
    return good, out


MUTATIONS = ("last row dropped", "last stage of the last split dropped", "one split counted twice", "lo*hi term dropped",
             "rows past a split's end taken from the next split", "clamped rows past the end not zeroed", "bias from the other 32-row block",
             "remap off by row_off")


@pytest.mark.parametrize("kind,M,remap", [("split", 2048 + 33, None), ("split", 2048 + 1, (7, 8, 1)), ("bf16", 2048 + 65, None), ("fp16", 2048 + 1, None),
                                          ("f32", 129, None), ("f32", 600, (7, 8, 1)), ("split", 600, None), ("bf16", 65, (7, 8, 1))])
def test_exact_comparison_flags_every_seeded_mistake(kind, M, remap):
    good, muts = mutants(kind, M, remap)
    assert set(muts) <= set(MUTATIONS)
    want = set(MUTATIONS) - ({"lo*hi term dropped"} if kind != "split" else set()) - ({"remap off by row_off"} if remap is None else set())
    if plan(kind, M, bias=True)["splits"] == 1:
        want -= {"rows past a split's end taken from the next split"}
    assert set(muts) == want, (set(muts) ^ want)
    gw, gb = good["dw"].float(), good["db"].float()
    for name, (dw, db) in muts.items():
        assert not (torch.equal(dw.float(), gw) and torch.equal(db.float(), gb)), f"{kind} M = {M}: '{name}' passes the exact comparison"
        if not name.startswith("bias"):
            assert not torch.equal(dw.float(), gw), name


# ---------------------------------------------------------------------------------------------------------------------------- Gaussian gate
@pytest.mark.parametrize("kind", R.KINDS)
def test_gaussian_gate_holds_for_f32_and_sees_a_dropped_row(kind):
    M = 2303
    dy, x = R.gauss_pair(kind, M, 128, 128)
    ref = R.reference(dy, x, kind)
    splits = plan(kind, M)["splits"]
    gate = R.gate_w(ref, kind, M, splits)
    err = (R.f32_shuffled(dy, x, kind).double() - ref["dw"]).abs()
    assert bool((err <= gate).all()), float((err / gate).max())
    assert float((err / gate).max()) < 0.05                    # an honest f32 sum sits far inside the worst-case bound ...
    dropped = R.reference(dy, x, kind, rows=torch.arange(M - 1))
    share = float(((dropped["dw"] - ref["dw"]).abs() > gate).double().mean())
    # ... and so the bound cannot see every dropped row: a product below 3 M 2^-24 of the element's abs-sum hides in it (35 % of the elements were
    # flagged at this shape when the gate was derived; the plain types' bound is three times tighter).  The exact cases are what catches a row.
    assert share > (0.2 if kind == "split" else 0.5), share
    assert bool(((dropped["db"] - ref["db"]).abs() > R.gate_b(ref, kind, M, splits)).double().mean() > 0.5)
