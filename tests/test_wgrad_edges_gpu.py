"""GPU: the weight-gradient GEMMs (csrc/gemm_tn2.hip: LDS-DMA ring; csrc/gemm.hip: gemm_tn_kernel; csrc/gemm_small.hip) through the single-op C entry
mfvit_linear_wgrad_ex / mfvit_linear_wgrad_pair at the edges of their split rule, element by element against the float64 reference of
tests/wgrad_ref.py:

  * EXACT inputs (every product and partial sum representable in f32): torch.equal with the reference - no tolerance.  One dropped, doubled or
    un-zeroed reduction row fails it (tests/test_wgrad_edges_cpu.py shows that for a list of seeded mistakes);
  * Gaussian inputs: every element inside the any-order bound of f32 accumulation (wgrad_ref.gate_w / gate_b);
  * every case first asserts what the launchers' plan reports for it (kernel, splits, rows of the last split, scratch, bias partials): the pins of
    wgrad_ref, so a change of the split rule fails here instead of moving the case to another edge;
  * every output sits inside NaN guard rows and columns (row pitch K + 4), dbias between NaN guards, the scratch starts as NaN.

The shapes are the smallest at which these kernels can go wrong: one 128 x 128 tile, M = 2,048 + r for the LDS-DMA kernel (the last split then holds r
rows: 1 .. 4 stages, fewer than the ring has slots, its last stage below / at / above one reduction half), M around KR and 4 KR for gemm_tn_kernel."""
import os

import pytest
import torch

import wgrad_ref as R
from mfvit import _lib, ops
from test_gemm_pp_gpu import REPORT as PP_REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT = os.path.join(os.path.dirname(PP_REPORT), "parity_wgrad_edges.txt")      # beside the tile GEMM's report: the suite's report directory
REMAP = (7, 8, 1)
# (scratch given, accumulate onto a pre-filled output, dbias: None / "aligned" (16 bytes: the bias partials) / "offset" (one float further: float atomics))
VARIANTS = [(False, False, None), (False, True, "aligned"), (False, False, "offset"), (True, False, None), (True, True, "aligned"), (True, True, "offset")]


def log(msg):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")


def plan(kind, M, N=128, K=128, **kw):
    return ops.linear_wgrad_plan(R.CODE[kind], M, N, K, **kw)


@pytest.fixture(autouse=True)
def whole_chip(monkeypatch):
    monkeypatch.delenv("MFVIT_TN_GLDS", raising=False)
    _lib.lib().mfvit_set_stream_share(1)
    yield
    _lib.lib().mfvit_set_stream_share(1)


_scratch = {}


def nan_scratch():
    if "t" not in _scratch:
        _scratch["t"] = torch.empty(ops.WGRAD_SCRATCH_FLOATS, device=DEV, dtype=torch.float32)
    _scratch["t"].fill_(float("nan"))
    return _scratch["t"]


def prefill(shape, seed):
    return torch.randint(-int(R.PREFILL), int(R.PREFILL) + 1, shape, generator=R.gen(seed)).float()


class Guarded:
    """an [N][K] f32 output inside two NaN guard rows above and below and four NaN guard columns (row pitch K + 4), or an [N] vector between NaN guards"""

    def __init__(self, N, K=None, pre=None, offset=0):
        if K is None:
            self.buf = torch.full((N + 12,), float("nan"), device=DEV)
            self.where = (slice(4 + offset, 4 + offset + N),)
        else:
            self.buf = torch.full((N + 4, K + 4), float("nan"), device=DEV)
            self.where = (slice(2, 2 + N), slice(0, K))
        self.view = self.buf[self.where]
        self.view.copy_(torch.zeros(self.view.shape) if pre is None else pre)
        self.before = self.buf.clone()

    def result(self):
        """the output on the CPU; asserts that every guard kept its bits"""
        after, before = self.buf.clone(), self.before.clone()
        after[self.where] = 0
        before[self.where] = 0
        assert torch.equal(after.view(torch.int32), before.view(torch.int32)), "a guard row / column / element was written"
        return self.view.cpu()


def describe(got, want):
    d = (got.double() - want.double())
    bad = d != 0
    bad |= torch.isnan(d)
    idx = bad.nonzero()
    return f"{int(bad.sum())} of {bad.numel()} elements differ, largest |diff| {float(d.abs().nan_to_num(float('inf')).max()):.6g}, first at {idx[0].tolist() if len(idx) else None}"


def launch(kind, dy_s, x_s, M, N, K, scratch=False, pre=False, bias=None, remap=None, seed=0):
    """one mfvit_linear_wgrad_ex launch on guarded outputs; returns (dw, db or None, pre_w, pre_b) as CPU tensors"""
    pre_w = prefill((N, K), 11 + seed) if pre else torch.zeros(N, K)
    pre_b = prefill((N,), 12 + seed) if pre else torch.zeros(N)
    out = Guarded(N, K, pre_w)
    db = Guarded(N, None, pre_b, offset=1 if bias == "offset" else 0) if bias else None
    if db is not None:
        assert (db.view.data_ptr() % 16 == 0) == (bias == "aligned")
    ops.linear_wgrad(dy_s, x_s, out=out.view, scratch=nan_scratch() if scratch else None, split=kind == "split", dbias=db.view if bias else None, remap=remap)
    torch.cuda.synchronize()
    return out.result(), (db.result() if bias else None), pre_w, pre_b


def to_dev(t, kind):
    return R.pack(t, kind).to(DEV)


def run_exact(kind, M, N=128, K=128, remap=None, variants=VARIANTS, pin=None):
    """every variant of one exact case: plan pins, bit equality of dW and dbias, guards.  Returns the outputs of the first variant."""
    dy, x, ref = R.exact_pair(kind, M, N, K, remap=remap, device=DEV)
    want_w, want_b = ref["dw"].float().cpu(), ref["db"].float().cpu()
    dy_s, x_s = to_dev(dy, kind), to_dev(x, kind)
    first = None
    for scratch, pre, bias in variants:
        p = plan(kind, M, N, K, bias=bias is not None, bias_aligned=bias != "offset", scratch=scratch, remap=remap is not None, lddw=K + 4)
        if pin is not None:
            multi = pin["splits"] > 1
            R.check_plan(p, pin, scratch and multi, scratch and multi and bias == "aligned")
        dw, db, pre_w, pre_b = launch(kind, dy_s, x_s, M, N, K, scratch, pre, bias, remap)
        tag = f"{kind} M={M} N={N} K={K} remap={remap} scratch={scratch} accumulate={pre} dbias={bias} plan={p}"
        assert torch.equal(dw, want_w + pre_w), f"dW {tag}: {describe(dw, want_w + pre_w)}"
        if bias:
            assert torch.equal(db, want_b + pre_b), f"dbias {tag}: {describe(db, want_b + pre_b)}"
        first = first or (dw, db)
    return first


def run_gauss(kind, M, N=128, K=128, scratch=True):
    dy, x = R.gauss_pair(kind, M, N, K)
    ref = R.reference(dy.to(DEV), x.to(DEV), kind)
    p = plan(kind, M, N, K, bias=True, scratch=scratch, lddw=K + 4)
    dw, db, _, _ = launch(kind, to_dev(dy, kind), to_dev(x, kind), M, N, K, scratch=scratch, bias="aligned")
    ew, eb = (dw.double() - ref["dw"].cpu()).abs(), (db.double() - ref["db"].cpu()).abs()
    gw, gb = R.gate_w(ref, kind, M, p["splits"]).cpu(), R.gate_b(ref, kind, M, p["splits"]).cpu()
    rw, rb = float((ew / gw).max()), float((eb / gb).max())
    log(f"gaussian {kind} {p['kernel']} M={M}: largest |err| / gate  dW {rw:.3e}  dbias {rb:.3e}  (gate = ({3 if kind == 'split' else 1} M + {p['splits']}) 2^-24 abs-sum)")
    assert bool((ew <= gw).all()) and bool((eb <= gb).all()), (kind, M, rw, rb)
    return rw, rb


# ------------------------------------------------------------------------------------------------------------------- LDS-DMA kernel
@pytest.mark.parametrize("kind", ["split", "bf16", "fp16"])
@pytest.mark.parametrize("i", range(14))
def test_lds_dma_last_split(kind, i):
    r = R.GLDS_R[kind][i]
    run_exact(kind, R.GLDS_M0 + r, pin=R.glds_pin(kind, r))
    log(f"exact lds-dma {kind} M=2048+{r}: {len(VARIANTS)} variants bit-equal, guards intact")


@pytest.mark.parametrize("kind", ["split", "bf16", "fp16"])
def test_lds_dma_stream_share_and_gaussian(kind):
    _lib.lib().mfvit_set_stream_share(2)
    for r in (1, 33):
        run_exact(kind, R.GLDS_M0 + r, pin=R.glds_pin(kind, r), variants=[(False, False, "aligned"), (True, True, "aligned")])
    _lib.lib().mfvit_set_stream_share(1)
    for r in (1, R.GLDS_KR[kind] + 1):
        assert plan(kind, R.GLDS_M0 + r)["kernel"] == "glds"
        run_gauss(kind, R.GLDS_M0 + r)
        run_gauss(kind, R.GLDS_M0 + r, scratch=False)
    log(f"exact lds-dma {kind} stream share 2, r in (1, 33): bit-equal")


@pytest.mark.parametrize("kind", ["split", "bf16", "fp16"])
@pytest.mark.parametrize("na,nb", [(128, 128), (384, 128)])
def test_lds_dma_pair(kind, na, nb):
    kr, e, K = R.GLDS_KR[kind], 2 if kind == "split" else 1, 128
    for r in (1, kr - 1, kr + 1):
        M = R.GLDS_M0 + r
        R.check_plan(plan(kind, M, na, K, N2=nb, bias=True, lddw=K + 4, lddw2=K + 4), R.glds_pin(kind, r, tiles=(na + nb) // 128), False, False)
        (dya, xa, ra), (dyb, xb, rb) = R.exact_pair(kind, M, na, K, device=DEV), R.exact_pair(kind, M, nb, K, seed=1, device=DEV)
        sa, sxa, sb, sxb = to_dev(dya, kind), to_dev(xa, kind), to_dev(dyb, kind), to_dev(xb, kind)
        for pre, bias in ((False, "aligned"), (True, "offset"), (True, None)):
            pa, pb, pbias = (prefill((na, K), 21), prefill((nb, K), 22), prefill((na,), 23)) if pre else (torch.zeros(na, K), torch.zeros(nb, K), torch.zeros(na))
            oa, ob = Guarded(na, K, pa), Guarded(nb, K, pb)
            db = Guarded(na, None, pbias, offset=1 if bias == "offset" else 0) if bias else None
            _lib.check(_lib.lib().mfvit_linear_wgrad_pair(R.CODE[kind], sa.data_ptr(), na * e, sxa.data_ptr(), K * e, oa.view.data_ptr(), K + 4,
                                                          db.view.data_ptr() if bias else None, na, sb.data_ptr(), nb * e, sxb.data_ptr(), K * e,
                                                          ob.view.data_ptr(), K + 4, nb, M, K, _lib.stream()), "mfvit_linear_wgrad_pair")
            torch.cuda.synchronize()
            ga, gb = oa.result(), ob.result()
            assert torch.equal(ga, ra["dw"].float().cpu() + pa), describe(ga, ra["dw"].float().cpu() + pa)
            assert torch.equal(gb, rb["dw"].float().cpu() + pb), describe(gb, rb["dw"].float().cpu() + pb)
            if bias:
                assert torch.equal(db.result(), ra["db"].float().cpu() + pbias)
            if not pre:     # the same bits as the two single launches
                s1 = launch(kind, sa, sxa, M, na, K, bias="aligned")
                s2 = launch(kind, sb, sxb, M, nb, K)
                assert torch.equal(ga, s1[0]) and torch.equal(db.result(), s1[1]) and torch.equal(gb, s2[0])
    log(f"exact lds-dma pair {kind} ({na}, {nb}) r in (1, {kr - 1}, {kr + 1}): both outputs and dbias bit-equal, equal to the single launches")


@pytest.mark.parametrize("kind", ["split", "bf16"])
@pytest.mark.parametrize("M", [2048, 2053])
def test_lds_dma_one_split(kind, M):
    """more tiles than half the target: one split, a given scratch stays unused and the result goes straight onto the accumulated output"""
    kr = R.GLDS_KR[kind]
    pin = dict(kernel="glds", kr=kr, splits=1, chunk=-(-M // kr) * kr, last_rows=M, tiles=144)
    run_exact(kind, M, 1536, 1536, pin=pin, variants=[(True, True, "aligned"), (False, False, None)])
    log(f"exact lds-dma {kind} M={M} N=K=1536 (one split): bit-equal")


@pytest.mark.parametrize("r", [1, 33])
def test_lds_dma_remap(r):
    """the patch-embedding form: rows_in = 7 of every 8 gradient rows, from row 1; the skipped rows hold NaN"""
    p = plan("split", R.GLDS_M0 + r, remap=True, scratch=True)
    assert p["kernel"] == "glds"
    run_exact("split", R.GLDS_M0 + r, remap=REMAP, pin=R.glds_pin("split", r), variants=[(False, False, None), (True, True, None), (False, True, None)])
    log(f"exact lds-dma remap split M=2048+{r}: bit-equal, NaN rows not read")


# ------------------------------------------------------------------------------------------------------------------- gemm_tn_kernel
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("i", range(8))
def test_tile_kernel(kind, i):
    M = R.tile_ms(kind)[i]
    variants = [v for v in VARIANTS if v[2] or kind != "f32" or M > 512]       # f32 up to 512 rows without bias sums goes to the small kernel
    run_exact(kind, M, pin=R.tile_pin(kind, M), variants=variants)
    if kind == "split":
        run_exact(kind, M, 64, 64, pin=R.tile_pin(kind, M, n=64))
    if M in (R.TILE_KR[kind] + 1, 600):
        run_exact(kind, M, remap=REMAP, pin=R.tile_pin(kind, M), variants=VARIANTS)      # (remapped rows: never the small kernel)
        run_gauss(kind, M)
    log(f"exact gemm_tn_kernel {kind} M={M}: bit-equal, guards intact")


def test_tile_kernel_tile_partials_without_bias_partials():
    pin = dict(kernel="tile", kr=32, splits=24, chunk=128, last_rows=128, tiles=16)
    p = plan("f32", 3072, 512, 512, bias=True, scratch=True, lddw=516)
    R.check_plan(p, pin, True, False)
    dy, x, ref = R.exact_pair("f32", 3072, 512, 512, device=DEV)
    dw, db, pre_w, pre_b = launch("f32", dy.to(DEV), x.to(DEV), 3072, 512, 512, scratch=True, pre=True, bias="aligned")
    assert torch.equal(dw, ref["dw"].float().cpu() + pre_w) and torch.equal(db, ref["db"].float().cpu() + pre_b)
    log("exact gemm_tn_kernel f32 M=3072 N=K=512 (384 tile partials, bias by atomics): bit-equal")


@pytest.mark.parametrize("kind", ["split", "bf16", "fp16"])
def test_tile_kernel_equals_lds_dma(kind, monkeypatch):
    for r in (1, 65):
        M = R.GLDS_M0 + r
        a = run_exact(kind, M, pin=R.glds_pin(kind, r), variants=[(True, False, "aligned"), (False, True, "offset")])
        monkeypatch.setenv("MFVIT_TN_GLDS", "0")
        b = run_exact(kind, M, pin=R.tile_pin(kind, M), variants=[(True, False, "aligned"), (False, True, "offset")])
        monkeypatch.delenv("MFVIT_TN_GLDS")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    log(f"exact {kind} M=2048+(1, 65): gemm_tn_kernel (MFVIT_TN_GLDS=0) and the LDS-DMA kernel give the same bits")


def test_small_kernel():
    assert plan("f32", 37)["kernel"] == "small"
    run_exact("f32", 37, variants=[(False, False, None), (True, True, None)])
    log("exact small f32 kernel M=37: bit-equal")


# ------------------------------------------------------------------------------------------------------------------- non-finite values
@pytest.mark.parametrize("kind,M,kernel,bias", [("split", 2048 + 33, "glds", "aligned"), ("bf16", 2048 + 65, "glds", "offset"), ("fp16", 2048 + 1, "glds", "aligned"),
                                                ("f32", 129, "tile", "aligned"), ("bf16", 65, "tile", "aligned"), ("split", 257, "tile", "offset"),
                                                ("f32", 37, "small", None)])
def test_non_finite_values_stay_in_their_row_and_column(kind, M, kernel, bias):
    """a partial last stage: the rows past M are fetched clamped to row M - 1 - what that row holds must reach its own column / row only"""
    N = K = 128
    assert plan(kind, M, bias=bias is not None, scratch=True)["kernel"] == kernel
    p = plan(kind, M, bias=True)
    assert p["kernel"] == "tile" or R.last_stage(p)[1] < p["kr"]
    dy, x, ref = R.exact_pair(kind, M, N, K, device=DEV)
    want_w, want_b = ref["dw"].float().cpu(), ref["db"].float().cpu()
    ks, ns = 37, 101
    for scratch in (False, True):
        xp = x.clone()
        xp[M - 1, ks] = float("inf")
        dw, db, _, _ = launch(kind, to_dev(dy, kind), to_dev(xp, kind), M, N, K, scratch=scratch, bias=bias)
        keep = torch.arange(K) != ks
        assert torch.equal(dw[:, keep], want_w[:, keep]), describe(dw[:, keep], want_w[:, keep])
        assert not bool(torch.isfinite(dw[:, ks]).any())
        if bias:
            assert torch.equal(db, want_b)
        dyp = dy.clone()
        dyp[M - 1, ns] = float("inf")
        dw, db, _, _ = launch(kind, to_dev(dyp, kind), to_dev(x, kind), M, N, K, scratch=scratch, bias=bias)
        keep = torch.arange(N) != ns
        assert torch.equal(dw[keep], want_w[keep]), describe(dw[keep], want_w[keep])
        assert not bool(torch.isfinite(dw[ns]).any())
        if bias:
            assert torch.equal(db[keep], want_b[keep]) and not bool(torch.isfinite(db[ns]))
    log(f"non-finite {kind} {kernel} M={M}: inf in X[M-1][{ks}] / dY[M-1][{ns}] stays in its column / row (and dbias entry)")


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    lib = _lib.lib()
    M, N, K = 600, 128, 128
    dy = torch.ones(M + 1, N + 8, device=DEV, dtype=torch.bfloat16)
    x = torch.ones(M + 1, K + 8, device=DEV, dtype=torch.bfloat16)
    out = Guarded(N, K, prefill((N, K), 31))
    db = Guarded(N, None, prefill((N,), 32))

    def ex(code, dy_p, lddy, x_p, ldx, m, n, k, remap=(0, 0, 0)):
        return lib.mfvit_linear_wgrad_ex(code, dy_p, lddy, x_p, ldx, out.view.data_ptr(), K + 4, m, n, k, None, db.view.data_ptr(), *remap, _lib.stream())

    b, h = R.CODE["bf16"], R.CODE["split"]
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr(), K + 8, M, N, K) == 0                       # (the control: a padded pitch of 16-byte multiples is taken)
    torch.cuda.synchronize()
    first = out.result()
    first_b = db.result()
    assert torch.equal(first, out.before[out.where].cpu() + M) and torch.equal(first_b, db.before[db.where].cpu() + M)
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr(), K + 8, M, 64, K) == -22                    # N * EP % 128
    assert ex(h, dy.data_ptr(), N + 8, x.data_ptr(), K + 8, M, 32, 64) == -22
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr(), K + 8, 0, N, K) == -22                     # M <= 0
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr(), K + 8, -5, N, K) == -22
    assert ex(b, dy.data_ptr(), N + 4, x.data_ptr(), K + 8, M, N, K) == -22                     # row pitch / base address not a multiple of 16 bytes
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr(), K + 4, M, N, K) == -22
    assert ex(b, dy.data_ptr() + 2, N + 8, x.data_ptr(), K + 8, M, N, K) == -22
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr() + 8, K + 8, M, N, K) == -22
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr(), K + 8, M, N, K, remap=(7, 7, 1)) == -22    # rows_out < rows_in + row_off
    assert ex(b, dy.data_ptr(), N + 8, x.data_ptr(), K + 8, M, N, K, remap=(0, 8, 1)) == -22
    big = torch.ones(2047, N, device=DEV, dtype=torch.bfloat16)
    assert lib.mfvit_linear_wgrad_pair(b, big.data_ptr(), N, big.data_ptr(), K, out.view.data_ptr(), K + 4, db.view.data_ptr(), N, big.data_ptr(), N,
                                       big.data_ptr(), K, out.view.data_ptr(), K + 4, N, 2047, K, _lib.stream()) == -38      # the pair below 2,048 rows
    torch.cuda.synchronize()
    assert torch.equal(out.result(), first) and torch.equal(db.result(), first_b)                # nothing was launched
    with pytest.raises(_lib.MfvitError):
        ops.linear_wgrad(dy[:M, :N], x[:M, :K], remap=(7, 8, 1))                                 # remapped rows past the end of dy: refused in the wrapper
    log("refusals: 12 shapes outside the domain return an error and leave the outputs untouched")
