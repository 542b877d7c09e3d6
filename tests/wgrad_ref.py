"""Reference, inputs and gates of the weight-gradient GEMM tests (tests/test_wgrad_edges_cpu.py, tests/test_wgrad_edges_gpu.py):

    dW[n][k] += sum_m dY[row(m)][n] X[m][k],    dbias[n] += sum_m dY[row(m)][n],    row(m) = (m // rows_in) * rows_out + m % rows_in + row_off

Reference: float64 on the ROUNDED operands.  Split bf16 stores a value as hi = bf16(v), lo = bf16(v - hi) and the kernels form the three products
hi*hi + hi*lo + lo*hi; the lo*lo they skip is not in the reference, so it is in no gate either.  The bias sums are sum_m (hi + lo).

Two kinds of input:
  * EXACT: operands on a grid on which every product and every partial sum is exactly representable in f32, so the f32 result is the same bits
    in ANY summation order - float atomics, split partials, two reduction halves added through LDS - and the comparison is torch.equal with the
    reference cast to f32: one dropped, doubled or un-zeroed row fails it.  Split bf16: {0, +-2, +-3} + l / 1024 with |l| <= 3 (l = 0 where the
    integer is 0), so hi is the integer, lo = l / 1024 exactly, and both parts carry data.  bf16 / fp16 / f32: integers in [-4, 4].  The condition
    on the data is checked for every generated pair (assert_exact): max over elements of sum_m (|ah xh| + |ah xl| + |al xh|), plus whatever the
    output held before, stays below 2^24 units of the smallest product unit (2^-10: the limit is 2^14; integers: 2^24).
  * GAUSSIAN: full hi / lo mantissas (dy * 0.1, x * 1.0 like the older tests), gated element by element by the any-order bound of f32
    accumulation, |out - ref| <= (3 M + splits) 2^-24 sum_m (|ah xh| + |ah xl| + |al xh|)   (plain types: (M + splits) 2^-24 sum |a x|), and the
    bias sums the same way over sum_m |a|.  Derived from the arithmetic (each of the 3 M products of an element enters one f32 add, each split one
    more), not from any kernel's output; no max-relative gate.
"""
import torch

KINDS = ("split", "bf16", "fp16", "f32")
CODE = {"f32": 0, "bf16": 1, "split": 2, "fp16": 3}                       # include/mfvit.h dtype codes
TDTYPE = {"split": torch.bfloat16, "bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
U = 2.0 ** -24                                                             # unit roundoff of f32


def gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_operand(g, shape, kind):
    """f32 values on the exact grid of `kind` (module docstring)."""
    if kind == "split":
        mag = torch.randint(2, 4, shape, generator=g).float()              # 2 or 3
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        keep = torch.randint(0, 2, shape, generator=g).float()             # half of the elements are 0
        h = mag * sign * keep
        lo = torch.randint(-3, 4, shape, generator=g).float() * (h != 0)
        return h + lo / 1024
    return torch.randint(-4, 5, shape, generator=g).float()


def gauss_operand(g, shape, scale):
    return torch.randn(shape, generator=g) * scale


def parts(t, kind):
    """(hi, lo) of the rounded operand as float64; lo is None for the plain types."""
    if kind == "split":
        hi = t.float().to(torch.bfloat16).float()
        lo = (t.float() - hi).to(torch.bfloat16).float()
        return hi.double(), lo.double()
    return t.float().to(TDTYPE[kind]).double(), None


def pack(t, kind):
    """Storage the kernels read: the plain type, or split bf16 [.., 2N] with every group of 32 columns as [hi x 32 | lo x 32]."""
    if kind != "split":
        return t.float().to(TDTYPE[kind]).contiguous()
    hi = t.float().to(torch.bfloat16)
    lo = (t.float() - hi.float()).to(torch.bfloat16)
    *lead, n = t.shape
    return torch.stack([hi.reshape(*lead, n // 32, 32), lo.reshape(*lead, n // 32, 32)], dim=-2).reshape(*lead, 2 * n).contiguous()


def remap_rows(M, remap, device="cpu"):
    """dY row of every reduction row m < M."""
    m = torch.arange(M, device=device)
    if remap is None:
        return m
    rin, rout, roff = remap
    return torch.div(m, rin, rounding_mode="floor") * rout + m % rin + roff


def remap_total(M, remap):
    """rows a dY tensor needs for M remapped reduction rows"""
    return int(remap_rows(M, remap)[-1]) + 1


def reference(dy, x, kind, remap=None, rows=None, drop_lohi=False):
    """dict(dw [N][K], db [N], absw, absb), float64, on the device of the inputs.  dy, x: f32 VALUES (rounded here); x has the M reduction rows, dy the
    rows remap_rows selects (its other rows are never read: they may hold NaN).  rows: optional index tensor - only these reduction rows are summed
    (the mutation checks).  drop_lohi: leave the lo*hi term out (a mutation)."""
    M = x.shape[0]
    idx = remap_rows(M, remap, dy.device)
    sel = torch.arange(M, device=dy.device) if rows is None else rows
    a = dy[idx[sel]]
    xx = x[sel]
    ah, al = parts(a, kind)
    xh, xl = parts(xx, kind)
    dw = ah.T @ xh
    db = ah.sum(0)
    if al is not None:
        dw = dw + ah.T @ xl
        if not drop_lohi:
            dw = dw + al.T @ xh
        db = db + al.sum(0)
    absw, absb = _abs_sums(ah, al, xh, xl)
    return dict(dw=dw, db=db, absw=absw, absb=absb)


def _abs_sums(ah, al, xh, xl):
    absw, absb = ah.abs().T @ xh.abs(), ah.abs().sum(0)
    if al is not None:
        absw, absb = absw + ah.abs().T @ xl.abs() + al.abs().T @ xh.abs(), absb + al.abs().sum(0)
    return absw, absb


def abs_sums(dy, x, kind, remap=None, dtype=torch.float64):
    """(sum_m |ah xh| + |ah xl| + |al xh| per element, sum_m |ah| + |al| per column): what the exactness condition and the gates are stated over"""
    c = lambda t: None if t is None else t.to(dtype)
    ah, al = parts(dy[remap_rows(x.shape[0], remap, dy.device)], kind)
    xh, xl = parts(x, kind)
    return _abs_sums(c(ah), c(al), c(xh), c(xl))


def exact_limit(kind):
    """2^24 units of the smallest product unit: 2^-10 on the split grid (hi * lo), 1 on the integer one"""
    return 2.0 ** 14 if kind == "split" else 2.0 ** 24


def assert_exact(ref, kind, pre_w=None, pre_b=None):
    """The exactness condition on the data (module docstring); pre_w / pre_b: what the outputs hold before the launch."""
    bw = ref["absw"] + (0 if pre_w is None else pre_w.double().abs().to(ref["absw"].device))
    bb = ref["absb"] + (0 if pre_b is None else pre_b.double().abs().to(ref["absb"].device))
    lim = exact_limit(kind)
    assert float(bw.max()) < lim and float(bb.max()) < lim, (kind, float(bw.max()), float(bb.max()), lim)
    return float(bw.max())


PREFILL = 8.0        # the accumulate cases start from integers in [-8, 8]
_PAIRS, _REFS = {}, {}


def exact_operands(kind, M, N, K, seed=0, remap=None):
    """(dy, x) of exact_pair without the reference"""
    key = (kind, M, N, K, seed, remap)
    if key not in _PAIRS:
        g = gen(1000 * seed + 7 * M + N + K + 13 * KINDS.index(kind))
        rows = M if remap is None else remap_total(M, remap)
        dy, x = exact_operand(g, (rows, N), kind), exact_operand(g, (M, K), kind)
        if remap is not None:
            skipped = torch.ones(rows, dtype=torch.bool)
            skipped[remap_rows(M, remap)] = False
            dy[skipped] = float("nan")
        _PAIRS[key] = (dy, x)
    return _PAIRS[key]


def exact_pair(kind, M, N, K, seed=0, remap=None, device="cpu"):
    """(dy, x, ref): f32 values on the exact grid (CPU tensors) and their reference on `device`, the same objects for the same arguments (cached, never
    modified: callers clone before they poison).  Remapped: dy has remap_total rows and the rows no reduction row reads hold NaN.  The exactness
    condition is asserted for every pair, with the largest pre-filled output on top."""
    key = (kind, M, N, K, seed, remap)
    dy, x = exact_operands(kind, M, N, K, seed, remap)
    rkey = key + (str(device),)
    if rkey not in _REFS:
        if len(_REFS) > 8:
            _REFS.clear()
        ref = reference(dy.to(device), x.to(device), kind, remap=remap)
        pre = torch.full((1,), PREFILL, device=device)
        ref["bound"] = assert_exact(ref, kind, pre_w=pre, pre_b=pre)
        _REFS[rkey] = ref
    return dy, x, _REFS[rkey]


def gauss_pair(kind, M, N, K, seed=0):
    g = gen(5000 + 1000 * seed + 7 * M + N + K + 13 * KINDS.index(kind))
    return gauss_operand(g, (M, N), 0.1), gauss_operand(g, (M, K), 1.0)


def gate_w(ref, kind, M, splits):
    """per-element bound of |dw - ref| (module docstring)"""
    return ((3 if kind == "split" else 1) * M + splits) * U * ref["absw"]


def gate_b(ref, kind, M, splits):
    return ((2 if kind == "split" else 1) * M + splits) * U * ref["absb"]


def f32_shuffled(dy, x, kind, seed=0, chunk=37):
    """dW accumulated in f32, the reduction rows in a shuffled order, in chunks, the three terms interleaved onto ONE accumulator: an honest f32
    summation in an order no kernel uses (CPU test: on exact inputs it equals the reference bit for bit, on Gaussian ones it sits inside the gate)."""
    ah, al = parts(dy, kind)
    xh, xl = parts(x, kind)
    f = lambda t: None if t is None else t.float()
    ah, al, xh, xl = f(ah), f(al), f(xh), f(xl)
    acc = torch.zeros(dy.shape[1], x.shape[1])
    for c in torch.randperm(x.shape[0], generator=gen(77 + seed)).split(chunk):
        acc = acc + ah[c].T @ xh[c]
        if al is not None:
            acc = acc + al[c].T @ xh[c]
            acc = acc + ah[c].T @ xl[c]
    return acc


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The directed cases and what the launchers' plan (mfvit_linear_wgrad_plan) must report for them.  The numbers are PINS, written down from the
# split rule as it stands: a change of the rule fails the pin (CPU and GPU) instead of silently moving the tests to other edges.
GLDS_KR = {"split": 32, "bf16": 64, "fp16": 64}
TILE_KR = {"split": 64, "bf16": 64, "fp16": 64, "f32": 32}
GLDS_M0 = 2048
# rows of the last split: last splits of 1 .. 4 stages (fewer than the ring has slots) whose last stage holds 1 row, one less than a reduction half
# (KR / 2), exactly one half, one more, all but one, and all
GLDS_R = {"split": (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127),
          "bf16": (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255),
          "fp16": (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255)}


def glds_pin(kind, r, tiles=1):
    """LDS-DMA kernel at M = 2,048 + r, up to 15 tiles: 2,048 rows in 16 splits of 128 (split bf16) / 8 of 256 (plain), and one more split of r rows"""
    chunk = 128 if kind == "split" else 256
    full = GLDS_M0 // chunk
    return dict(kernel="glds", kr=GLDS_KR[kind], splits=full + (r > 0), chunk=chunk, last_rows=r if r else chunk, tiles=tiles)


def tile_ms(kind):
    kr = TILE_KR[kind]
    return (1, kr - 1, kr, kr + 1, 4 * kr, 4 * kr + 1, 600, 2047)


# gemm_tn_kernel, one to four storage tiles (N = K = 128; split bf16 also N = K = 64): M -> (splits, chunk, last_rows).  At least four stages per split.
TILE_PIN = {
    32: {1: (1, 32, 1), 31: (1, 32, 31), 32: (1, 32, 32), 33: (1, 64, 33), 128: (1, 128, 128), 129: (2, 96, 33), 600: (5, 128, 88), 2047: (16, 128, 127)},
    64: {1: (1, 64, 1), 63: (1, 64, 63), 64: (1, 64, 64), 65: (1, 128, 65), 256: (1, 256, 256), 257: (2, 192, 65), 600: (3, 256, 88), 2047: (8, 256, 255),
         2049: (9, 256, 1), 2113: (9, 256, 65)},
}


def tile_pin(kind, M, n=128):
    """n = N = K; the tile grid runs over STORAGE columns: split bf16 has four 128 x 128 storage tiles at n = 128 and one at n = 64"""
    s, c, l = TILE_PIN[TILE_KR[kind]][M]
    tiles = (n * (2 if kind == "split" else 1) // 128) ** 2
    return dict(kernel="tile", kr=TILE_KR[kind], splits=s, chunk=c, last_rows=l, tiles=tiles)


def check_plan(plan, pin, scratch, kpart):
    """the plan entry's report against a pin; scratch / kpart: whether the partials must go through the scratch / the bias rows behind them"""
    got = {k: plan[k] for k in pin}
    assert got == pin and plan["scratch"] == scratch and plan["kpart"] == kpart, (plan, pin, scratch, kpart)


def last_stage(plan):
    """(first row, valid rows) of the last stage of the last split"""
    last0 = (plan["splits"] - 1) * plan["chunk"]
    st = (plan["last_rows"] - 1) // plan["kr"]
    return last0 + st * plan["kr"], plan["last_rows"] - st * plan["kr"]
