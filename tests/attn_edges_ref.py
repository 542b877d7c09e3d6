"""The case table, the inputs and the float64 references of tests/test_attn_edges_cpu.py and tests/test_attn_edges_gpu.py: the attention
core (mfvit_attention_fwd / _bwd) at the sequence lengths, head widths and pair counts where the host switches from one kernel family to the
next, and on PEAKED logits (a few keys far above the rest, as trained heads have them) instead of the N(0, 1) logits of every other attention
test.  Not a test module.

Which family a call takes is decided on the host (csrc/attention.hip::attn_route, attention_mfma.hip::plan_fwd_t / plan_bwd_t,
attention_tiled.hip::tl_plan) and reported by mfvit_attention_plan.  `expect()` below restates those decisions from the launchers' formulas in
plain Python; every case also NAMES the families it was chosen for, by hand.  The CPU file asserts that the three agree.

Modes: the four of test_precision_gpu.py::ATT_MODES plus fp32 (the exact kernels).  Tolerances are the project's own:
  out   mode.tol  (5e-5 split, 1.5e-3 fp16, 8e-3 bf16; fp32 3e-5 as test_ops_gpu.py)       lse   1e-5
  dq / dk / dv / dbias   test_precision_gpu.py::bwd_tol  (2e-4 bf16x3, 1e-3 x3f16, 4e-3 fp16, 2e-2 bf16; fp32 3e-5)
all as max |got - ref| / max |ref|; dq, dk and dv are each judged against max |ref| of the whole dqkv (at T = 1 the references of dq and dk are
exactly 0: the softmax of one key has no derivative).

References (float64, on whatever device the operands live on):
  forward   on the rounded operands (mode.rounded_qkv)
  backward  on what the kernel is given - the STORED out, the STORED lse and the rounded dout:
            P = exp(s - lse), D = rowsum(dout o out), dS = P o (dP - D), dq = scale dS k, dk = scale dS^T q, dv = P^T dout, dbias = column sums
            (attention dropout: dP and the P of dv carry keep / (1 - p)).

Peaked inputs: q, k, v ~ randn, except coordinate 0 of every head: q_0 = a_i beta, k_0 = g_j beta with beta^2 / sqrt(d) = step, so that logit
(i, j) gains a_i g_j step.  a_i = 0 for the rows 0 .. 31 (one row tile never rescales) and cycles +1, -1, 0 from row 32 on; g_j is constant on
a 32-key tile: jump(t): 1 in key tile t, else 0; stairs: +1 from tile 2, +2 from tile 5.  The persistent forward (attn_fwd_pp_kernel) takes tile 0's
row maximum as the softmax reference and rescales only when a later tile exceeds it by AttnT::LAZY in log2: 14 (9.70 nats) for split fp16, 24
(16.64 nats) for split bf16.  step 6 crosses neither, 13 the first only (stairs: the second once, from a reference 13 stale), 21 both.  Each
peaked case declares the crossings of its a = +1 rows at the two thresholds; test_attn_edges_cpu.py counts them on the float64 logits.
stairs at step 6 is left out: its second stair stands 12 above the reference, 2.3 over the first threshold - whether a row crosses then hangs
on its noise."""
import collections
import functools
import math
import os

import torch

import test_precision_gpu as TP

EINVAL, ENOSYS = -22, -38
LDS_LIMIT = 160 * 1024
LN2 = math.log(2.0)
LAZY_LOG2 = {"x3f16": 14.0, "bf16x3": 24.0}          # csrc/attention_mfma.hip: AttnT<T>::LAZY
REPORT = os.path.join(os.path.dirname(TP.REPORT), "parity_attention_edges.txt")      # the directory of the other parity logs


def log(msg):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")


# ------------------------------------------------------------------------------------------------------------------------------------ modes
class Fp32Mode(TP.Mode):
    """The exact kernels (csrc/attention.hip): f32 storage, f32 arithmetic."""

    def __init__(self):
        self.name, self.split, self.tol = "fp32", False, 3e-5

    def pack(self, x):
        return x.float().to(TP.dev())

    def rounded(self, x):
        return x.float().double()


MODES = {m.name: m for m in TP.ATT_MODES + [Fp32Mode()]}
CODE = {"fp32": 0, "bf16": 1, "bf16x3": 2, "fp16": 3, "x3f16": 4}                       # include/mfvit.h: MFVIT_F32 ...
ALL5 = ("bf16x3", "fp16", "bf16", "x3f16", "fp32")
LSE_TOL = 1e-5


def bwd_tol(mode):
    return 3e-5 if mode.name == "fp32" else TP.bwd_tol(mode)


# --------------------------------------------------------------------------------------------------- the launchers' decisions, restated
def tpad(T):
    return (T + 31) & ~31


def tiles(T):
    return (T + 31) >> 5


def _mfma_supported(split, T, d, backward):
    """attention_mfma.hip::attn_mfma_supported: the whole head in LDS (head_dim 32 only)."""
    if d != 32 or T < 1:
        return False
    rb, tp = (128 if split else 64), tpad(T)
    if backward:
        if tp * (rb // 16) > 4 * 512:
            return False
        return 4 * tp * rb + 2 * tp * 4 + tp * rb + 64 <= LDS_LIMIT
    return tp * (rb + 16) + tp * rb <= LDS_LIMIT


def qkv_code(mode_name, T, d):
    """attention.hip::attn_qkv_dtype for the activations of a mode: X3F16 for BF16X3 where both whole-head directions apply."""
    if mode_name == "bf16x3" and _mfma_supported(True, T, d, False) and _mfma_supported(True, T, d, True):
        return CODE["x3f16"]
    return CODE[mode_name]


def expect(mode_name, B, T, H, d, backward, cus=256, bwd_sp=True):
    """dict(family, tiles, lds, grid, threads, lds2) of the launch, or the error code of the refusal."""
    if mode_name == "fp32":
        if d not in (32, 64):
            return EINVAL
        lds = 2 * T * d * 4 + (2 * T * 4 if backward else 0)                         # K, V as f32 (+ the D and lse rows)
        return EINVAL if lds > LDS_LIMIT else dict(family="exact", tiles=0, lds=lds, grid=B * H, threads=256, lds2=0)
    split = mode_name in ("bf16x3", "x3f16")
    if not _mfma_supported(split, T, d, backward):
        if mode_name == "x3f16":
            return ENOSYS
        if d not in (32, 64, 96):
            return EINVAL
        lds = 2 * 64 * (d * 2 * (2 if split else 1) + 16)                             # two 64-row chunks at the padded pitch
        return dict(family="stream", tiles=tiles(T), lds=lds, grid=B * H * ((T + 127) // 128), threads=256,
                    lds2=lds + 2 * 64 * 4 if backward else 0)
    rb, tp, nt = (128 if split else 64), tpad(T), tiles(T)
    rpp = 64 // (rb // 16)                                                            # rows of one 1-KB LDS-DMA piece
    timg = (T + rpp - 1) // rpp * rpp
    if not backward:
        ring = 2 * 2 * timg * rb + (tp - timg) * rb + 7 * 32 * (rb + 16)              # RingGeo::lds_bytes
        if split and B * H >= 2 * cus and 5 <= nt <= 7 and ring <= LDS_LIMIT:
            return dict(family="fwd_pp", tiles=nt, lds=ring, grid=cus, threads=512, lds2=0)
        return dict(family="pair", tiles=nt, lds=tp * (rb + 16 + rb), grid=B * H, threads=256, lds2=0)
    wide = 4 * tp * (rb + 16) + 2 * tp * 4 + tp * rb + 64 <= LDS_LIMIT
    sp = 4 * timg * rb + 2 * 7 * 32 * rb + 2 * tp * 4 + 32                            # SpGeo::lds_bytes
    if bwd_sp and B * H >= 2 * cus and nt == 7 and sp <= LDS_LIMIT:
        return dict(family="bwd_sp", tiles=nt, lds=sp, grid=cus, threads=512, lds2=0)
    return dict(family="bwd_padded" if wide else "bwd_unpadded", tiles=nt, lds=4 * tp * (rb + 16 if wide else rb) + 2 * tp * 4 + tp * rb,
                grid=min(B * H, cus), threads=512, lds2=0)


# -------------------------------------------------------------------------------------------------------------------------------- the cases
# plain / split: the (forward, backward) families the case was chosen for in the plain 16-bit types and in split bf16, named by hand (None:
# refused).  x3f16 takes the split pair where it is accepted (head_dim 32: both directions to T = 224, the forward alone to 576), fp32 the exact kernels.
# peak: None (randn) or (pattern, tile, step); cross: the lazy rescales of an a = +1 row at the thresholds (9.70, 16.64).  drop: attention dropout.
# Rejected seeds (test_attn_edges_cpu.py::test_peaked_cases_take_the_rescales_they_declare): pp192-stairs-13 7088 and pair197-jump3-13 7110 - one
# a = +1 row each whose tile-0 maximum stands so far above the jump tile's noise that the 13 do not carry it over 9.70; reseed = 1 takes the next.
Case = collections.namedtuple("Case", "name B T H d modes plain split why peak cross drop seed", defaults=(None, None, 0.0, 0))
PP, PAD, UNP, SP, STR, PAIR = "fwd_pp", "bwd_padded", "bwd_unpadded", "bwd_sp", "stream", "pair"


def _boundary_cases():
    out = []

    def add(T, d, modes, plain, split, why, B=None):
        H = {32: 12, 64: 6, 96: 4}[d]
        B = B or (2 if T <= 257 else 1)
        out.append(Case(f"d{d}-T{T}" + (f"-B{B}" if B > 2 else ""), B, T, H, d, modes, plain, split, why, seed=5000 + 7 * len(out)))
    whole, str_bwd, str_all = (PAIR, PAD), (PAIR, STR), (STR, STR)
    for T, plain, split, why in (
            (1, whole, whole, "one token: one key, 31 masked"), (2, whole, whole, "a 16 x 16 image"),
            (31, whole, whole, "one short of a tile"), (32, whole, whole, "exactly one tile"), (33, whole, whole, "one row into a second tile"),
            (128, whole, whole, "four tiles: below the persistent forward"), (129, whole, whole, "five tiles, few pairs"),
            (224, whole, whole, "last T of the split whole-head backward and of X3F16"),
            (225, whole, str_bwd, "split: streaming backward; qkv tag back to BF16X3"),
            (256, whole, str_bwd, "a 128-row block boundary of the streaming backward"), (257, whole, str_bwd, "one row into the third block"),
            (384, whole, str_bwd, "twelve tiles"), (385, whole, str_bwd, "one row into the 13th tile"),
            (416, whole, str_bwd, "last T of the padded backward images"), (417, (PAIR, UNP), str_bwd, "first T of the unpadded images (Tpad 448)"),
            (448, (PAIR, UNP), str_bwd, "unpadded images, full tiles"), (449, (PAIR, UNP), str_bwd, "unpadded images, Tpad 480"),
            (480, (PAIR, UNP), str_bwd, "last T of the whole-head backward"), (481, str_bwd, str_bwd, "plain: streaming backward"),
            (576, str_bwd, str_bwd, "last T of the split per-pair forward"), (577, str_bwd, str_all, "split: streaming forward"),
            (1120, str_bwd, str_all, "last T of the plain per-pair forward"), (1121, str_all, str_all, "plain: streaming forward")):
        add(T, 32, ALL5, plain, split, why)
    for T, why in ((620, "last T of the exact backward"), (621, "exact backward refused, forward runs"), (640, "last T of the exact forward"),
                   (641, "exact forward refused")):
        add(T, 32, ("fp32",), None, None, why)
    for T in (64, 65, 127, 128, 129):
        add(T, 64, ("bf16x3", "fp16", "bf16", "fp32"), str_all, str_all, "head_dim 64: streaming at a chunk / block edge")
    for T, why in ((315, "last T of the exact backward"), (316, "exact backward refused"), (320, "last T of the exact forward"), (321, "refused")):
        add(T, 64, ("fp32",), None, None, "head_dim 64: " + why)
    for T in (63, 64, 65, 128, 129, 193):
        add(T, 96, ("bf16x3", "fp16", "bf16"), str_all, str_all, "head_dim 96: streaming at a chunk / block edge")
    # the pair-count gate of the persistent forward and the single-pass backward: B * H = 504 and 516 around 2 x 256 CUs
    for T, plain, split, why in ((128, whole, whole, "four tiles: neither persistent kernel"), (129, whole, (PP, PAD), "five tiles"),
                                 (192, whole, (PP, PAD), "six tiles"), (193, (PAIR, SP), (PP, SP), "seven tiles, one row in the last"),
                                 (224, (PAIR, SP), (PP, PAD), "seven full tiles: the split single-pass images no longer fit")):
        add(T, 32, ALL5, whole, whole, "504 pairs, below the gate: " + why, B=42)
        add(T, 32, ALL5, plain, split, "516 pairs, above the gate: " + why, B=43)
    return tuple(out)


def _peaked_cases():
    out = []

    def add(name, B, T, d, peak, cross, plain, split, why, modes=ALL5, drop=0.0, reseed=0):
        H = {32: 12, 64: 6, 96: 4}[d]
        out.append(Case("peak-" + name, B, T, H, d, modes, plain, split, why, peak, cross, drop, seed=7000 + 11 * len(out) + 1000 * reseed))
    big, big224, small = ((PAIR, SP), (PP, SP)), ((PAIR, SP), (PP, PAD)), ((PAIR, PAD), (PAIR, PAD))
    # persistent forward and single-pass backward: 516 pairs
    add("pp197-jump1-6", 43, 197, 32, ("jump", 1, 6), (0, 0), *big, "no threshold crossed")
    add("pp197-jump3-13", 43, 197, 32, ("jump", 3, 13), (1, 0), *big, "split fp16 rescales in a middle step")
    # (the 5 keys of tile 6 stand 21 above the rest, their maximum 4.4 - its noise above the second threshold: of 28,380 rows a handful stay
    # below it with every seed tried, so the count at 16.64 is not declared - None - and only the first is checked)
    add("pp197-jump6-21", 43, 197, 32, ("jump", 6, 21), (1, None), *big, "rescale in last_step, on a tile of 5 keys")
    add("pp197-stairs-13", 43, 197, 32, ("stairs", 0, 13), (2, 1), *big, "split bf16 crosses once, from a reference 13 stale")
    add("pp197-stairs-21", 43, 197, 32, ("stairs", 0, 21), (2, 2), *big, "two rescales each; the largest logits")
    add("pp224-jump6-13", 43, 224, 32, ("jump", 6, 13), (1, 0), *big224, "last_step on a full tile")
    add("pp224-stairs-21", 43, 224, 32, ("stairs", 0, 21), (2, 2), *big224, "seven full tiles")
    add("pp160-jump4-21", 43, 160, 32, ("jump", 4, 21), (1, 1), (PAIR, PAD), (PP, PAD), "five tiles: the rescale in last_step")
    add("pp192-stairs-13", 43, 192, 32, ("stairs", 0, 13), (2, 1), (PAIR, PAD), (PP, PAD), "six tiles", reseed=1)
    # the per-pair kernels
    add("pair197-stairs-21", 2, 197, 32, ("stairs", 0, 21), (2, 2), *small, "per-pair forward, two-phase backward")
    add("pair197-jump3-13", 2, 197, 32, ("jump", 3, 13), (1, 0), *small, "the jump inside the first 4-tile chunk", reseed=1)
    # both forms of the two-phase backward (plain types; the split types stream their backward here)
    add("T416-stairs-21", 2, 416, 32, ("stairs", 0, 21), (2, 2), (PAIR, PAD), (PAIR, STR), "padded images at their last T")
    add("T448-stairs-21", 2, 448, 32, ("stairs", 0, 21), (2, 2), (PAIR, UNP), (PAIR, STR), "unpadded images")
    add("T448-jump13-13", 2, 448, 32, ("jump", 13, 13), (1, 0), (PAIR, UNP), (PAIR, STR), "unpadded images, the jump in the last tile")
    # streaming
    add("T225-stairs-21", 2, 225, 32, ("stairs", 0, 21), (2, 2), (PAIR, PAD), (PAIR, STR), "split streaming backward, one row in the last tile")
    add("d64-T129-stairs-13", 2, 129, 64, ("stairs", 0, 13), (1, 0), (STR, STR), (STR, STR), "head_dim 64, the third chunk holds one key",
        modes=("bf16x3", "fp16", "bf16", "fp32"))
    add("d96-T129-jump3-21", 2, 129, 96, ("jump", 3, 21), (1, 1), (STR, STR), (STR, STR), "head_dim 96", modes=("bf16x3", "fp16", "bf16"))
    add("d96-T129-stairs-21-drop", 2, 129, 96, ("stairs", 0, 21), (1, 1), (STR, STR), (STR, STR), "head_dim 96 with attention dropout 0.1",
        modes=("bf16x3", "fp16", "bf16"), drop=0.1)
    return tuple(out)


BOUNDARY = _boundary_cases()
PEAKED = _peaked_cases()
CASES = BOUNDARY + PEAKED
BY_NAME = {c.name: c for c in CASES}
GATE = tuple(c for c in BOUNDARY if c.B > 2)
DROP_SEED, DROP_SITE = 0x1234_5678_9ABC, 7


# refused calls: (mode, B, T, H, d, backward, code)
REFUSALS = (("x3f16", 1, 225, 12, 32, True, ENOSYS), ("x3f16", 1, 577, 12, 32, False, ENOSYS),       # (its forward alone runs up to T = 576)
            ("fp32", 1, 621, 12, 32, True, EINVAL), ("fp32", 1, 316, 6, 64, True, EINVAL),
            ("fp32", 1, 641, 12, 32, False, EINVAL), ("fp32", 1, 321, 6, 64, False, EINVAL),
            ("fp32", 1, 65, 4, 96, False, EINVAL), ("fp32", 1, 65, 4, 96, True, EINVAL))


def named_families(case, mode_name):
    """(forward, backward) family the case names for a mode; None in a direction the launch refuses."""
    e = [expect(mode_name, case.B, case.T, case.H, case.d, bw) for bw in (False, True)]
    if mode_name == "fp32":
        return tuple(None if isinstance(x, int) else "exact" for x in e)
    if mode_name == "x3f16":
        return tuple(None if isinstance(x, int) else f for x, f in zip(e, case.split))
    return case.split if mode_name == "bf16x3" else case.plain


def runs(case, mode_name, backward=False):
    return mode_name in case.modes and not isinstance(expect(mode_name, case.B, case.T, case.H, case.d, backward), int)


def pairs(cases, backward=False):
    """(case, mode name) of every launch that is accepted in the given direction, with its pytest id."""
    return [(c, m) for c in cases for m in c.modes if runs(c, m, backward)]


def pair_ids(ps):
    return [f"{c.name}-{m}" for c, m in ps]


# ------------------------------------------------------------------------------------------------------------------------------- the inputs
def peak_profile(case):
    """(a [T], g [T]): the row signs and the key levels of a peaked case."""
    kind, tile, _ = case.peak
    i = torch.arange(case.T)
    a = torch.tensor([1.0, -1.0, 0.0])[(i - 32) % 3] * (i >= 32)
    t = i // 32
    g = (t == tile).double() if kind == "jump" else (t >= 2).double() + (t >= 5).double()
    return a.double(), g


@functools.lru_cache(maxsize=4)
def inputs(name):
    """(qkv [B, T, 3 H d], dout [B, T, H d]) of a case, f32 on the CPU: randn drawn sample by sample (the first samples of a large batch are
    the inputs of the same case at a smaller one); peaked cases overwrite coordinate 0 of q and k of every head."""
    c = BY_NAME[name]
    D = c.H * c.d
    qkv, dout = torch.empty(c.B, c.T, 3 * D), torch.empty(c.B, c.T, D)
    for b in range(c.B):
        gen = torch.Generator().manual_seed(c.seed * 131 + b)
        qkv[b] = torch.randn(c.T, 3 * D, generator=gen)
        dout[b] = torch.randn(c.T, D, generator=gen)
    if c.peak is not None:
        a, g = peak_profile(c)
        beta = math.sqrt(c.peak[2] * math.sqrt(c.d))
        v = qkv.view(c.B, c.T, 3, c.H, c.d)
        v[:, :, 0, :, 0] = (a * beta).float()[None, :, None]
        v[:, :, 1, :, 0] = (g * beta).float()[None, :, None]
    return qkv, dout


def randn_twin(case):
    """The same shape and draws without the peaks."""
    c = case._replace(peak=None)
    D = c.H * c.d
    qkv = torch.empty(c.B, c.T, 3 * D)
    for b in range(c.B):
        qkv[b] = torch.randn(c.T, 3 * D, generator=torch.Generator().manual_seed(c.seed * 131 + b))
    return qkv


# --------------------------------------------------------------------------------------------------------------------------- the references
def heads(x, H, n):
    """[B, T, n H d] -> n tensors [B, H, T, d] (float64)."""
    B, T, W = x.shape
    return x.double().reshape(B, T, n, H, W // (n * H)).permute(2, 0, 3, 1, 4)


def merge(x):
    B, H, T, d = x.shape
    return x.transpose(1, 2).reshape(B, T, H * d)


def logits(qkv, H):
    q, k, _ = heads(qkv, H, 3)
    return (q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5


def ref_fwd(qkv, H, keep=None, p=0.0):
    """(out [B, T, D], lse [B, H, T]) in float64 of the operands as given.  keep [B, H, T, T]: the dropout mask on the probabilities."""
    q, k, v = heads(qkv, H, 3)
    s = (q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    if keep is not None:
        P = P * keep.double() / (1.0 - p)
    return merge(P @ v), lse


def ref_bwd(qkv, out, lse, dout, H, keep=None, p=0.0):
    """(dqkv [B, T, 3 D], dbias [3 D]) in float64 from the forward's stored out and lse."""
    q, k, v = heads(qkv, H, 3)
    o, do = heads(out, H, 1)[0], heads(dout, H, 1)[0]
    scale = q.shape[-1] ** -0.5
    P = torch.exp((q @ k.transpose(-1, -2)) * scale - lse.double()[..., None])
    m = 1.0 if keep is None else keep.double() / (1.0 - p)
    dP = (do @ v.transpose(-1, -2)) * m
    D = (do * o).sum(-1, keepdim=True)
    dS = P * (dP - D)
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), (P * m).transpose(-1, -2) @ do
    B, Hh, T, d = q.shape
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * Hh * d)
    return dqkv, dqkv.sum((0, 1))


def scale_err(got, ref, denom=None):
    """max |got - ref| / max |ref| (or / denom), on the reference's device."""
    ref = ref.double()
    got = got.double().to(ref.device)
    d = ref.abs().max().clamp_min(1e-300) if denom is None else denom
    return float((got - ref).abs().max() / d)


def dqkv_errs(got, ref, B, T):
    """Errors of dq, dk, dv, each against the largest |ref| of the whole dqkv."""
    den = ref.abs().max().clamp_min(1e-300)
    g, r = got.double().to(ref.device).view(B, T, 3, -1), ref.view(B, T, 3, -1)
    return [float((g[:, :, i] - r[:, :, i]).abs().max() / den) for i in range(3)]


# ------------------------------------------------------------------------------------- the lazy maximum: crossings and a rounding model
def lazy_crossings(s, thr):
    """Per row of the logits s [..., T, T] (nats): how often a key tile's maximum exceeds the running reference (tile 0's maximum, moved to the
    running maximum at every crossing) by more than thr."""
    T = s.shape[-1]
    m = s[..., :32].max(-1).values
    n = torch.zeros_like(m, dtype=torch.long)
    for t in range(1, tiles(T)):
        cm = s[..., 32 * t:32 * t + 32].max(-1).values
        fire = cm > m + thr
        n += fire
        m = torch.where(fire, torch.maximum(m, cm), m)
    return n


def round_parts(p, mode_name):
    """P as the second product of a split mode sees it: two 16-bit parts of the f32 value (fp16: inf past 65504)."""
    dt = torch.float16 if mode_name == "x3f16" else torch.bfloat16
    p32 = p.float()
    hi = p32.to(dt)
    lo = (p32 - hi.float()).to(dt)
    return hi.double() + lo.double()


def emulate_lazy(qkv, H, mode_name, mutant=None):
    """float64 emulation of the tile-wise lazy-maximum forward (attn_fwd_pp_kernel::step): per 32-row tile and 32-key tile, rescale o and lsum
    when ANY row of the row tile exceeds its reference by LAZY (the kernel's wave-wide ballot), p = exp2(s - m) summed unrounded into lsum and
    rounded to the mode's two operand parts for P V.  mutant: 'skip_o' / 'skip_lsum' leave that rescale out, 'never': no rescale behind tile 0.
    Returns (out, lse)."""
    q, k, v = heads(qkv, H, 3)
    B, Hh, T, d = q.shape
    s2 = (q @ k.transpose(-1, -2)) * (d ** -0.5 / LN2)                                # log2 units
    lazy = LAZY_LOG2[mode_name]
    m2 = torch.full((B, Hh, T), -math.inf, dtype=torch.float64)
    lsum = torch.zeros(B, Hh, T, dtype=torch.float64)
    o = torch.zeros(B, Hh, T, d, dtype=torch.float64)
    nt, Tp = tiles(T), tpad(T)
    for t in range(nt):
        st = s2[..., 32 * t:32 * t + 32]
        cm = st.max(-1).values
        fire = cm > m2 + lazy
        if mutant == "never" and t > 0:
            fire = torch.zeros_like(fire)
        pad = torch.zeros(B, Hh, Tp, dtype=torch.bool)
        pad[..., :T] = fire
        fire = pad.view(B, Hh, nt, 32).any(-1, keepdim=True).expand(B, Hh, nt, 32).reshape(B, Hh, Tp)[..., :T]
        mn = torch.where(fire, torch.maximum(m2, cm), m2)
        alpha = torch.exp2(m2 - mn)
        if mutant != "skip_lsum":
            lsum = lsum * alpha
        if mutant != "skip_o":
            o = o * alpha[..., None]
        m2 = mn
        p = torch.exp2(st - m2[..., None])
        lsum = lsum + p.sum(-1)
        o = o + round_parts(p, mode_name) @ v[..., 32 * t:32 * t + 32, :]
    return merge(o / lsum[..., None]), (m2 + torch.log2(lsum)) * LN2


def meets(out, lse, o_ref, l_ref, tol):
    """Finite and inside the output and lse tolerances."""
    if not (bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())):
        return False
    return scale_err(out, o_ref) < tol and scale_err(lse, l_ref) < LSE_TOL


# ------------------------------------------------------------------------------- the split-bf16 format on peaked logits: a rounding model
# A product of two split-bf16 tensors runs as hi hi + lo hi + hi lo: the lo lo term, 2^-18 of |a| |b|, is dropped.  On randn operands that is
# 2^-18 of a logit of order 1.  At the second stair of step 21 the product q_0 k_0 = 2 beta^2 = 238 alone puts up to 238 x 2^-18 x scale = 1.6e-4
# on a logit, different from key to key - and P = exp(s - lse) carries it as a RELATIVE error into dS and from there into dk (the sum over the rows
# with q_0 = +-beta).  The forward hides it (out 8e-6: the normaliser has the same error), the stored lse shows it (4.5e-6 of 47), and dk of the two
# T = 197 stairs-21 cases comes out at 2.1e-4, over test_precision_gpu.py's 2e-4 - in the single-pass, the two-phase and (T = 225: 1.99e-4) the
# streaming backward alike.  model_bf16x3 below is that arithmetic in float64 with nothing else in it: exact sums, P and dS rounded to two
# bf16 parts, results rounded to split storage.  It lands on the kernels' figures to two digits, so the format alone explains the miss, and the dk
# bound of exactly these two (case, mode) pairs is 2 x the model's error (the rule of the issue these tests answer; every other bound, and dq, dv
# and dbias of these two, stay the project's).  model: the model's dk error (test_attn_edges_cpu.py recomputes it); measured: the kernel's.
MODEL_BOUNDS = {("peak-pp197-stairs-21", "bf16x3"): dict(model=2.08e-4, measured=2.09e-4),        # fwd_pp / bwd_sp
                ("peak-pair197-stairs-21", "bf16x3"): dict(model=2.09e-4, measured=2.10e-4)}      # pair / bwd_padded


def dk_bound(case, mode):
    m = MODEL_BOUNDS.get((case.name, mode.name))
    return 2.0 * m["model"] if m else bwd_tol(mode)


def bf16_parts(x):
    x32 = x.float()
    hi = x32.bfloat16()
    return hi.double(), (x32 - hi.float()).bfloat16().double()


def prod3(a, b):
    """a @ b of two split-bf16 operands as the kernels multiply them: hi hi + lo hi + hi lo, summed exactly."""
    ah, al = bf16_parts(a)
    bh, bl = bf16_parts(b)
    return ah @ bh + al @ bh + ah @ bl


def model_bf16x3(qkv, dout, H):
    """The split-bf16 forward and backward in float64 with the format's roundings only.  Returns (out error, lse error, [dq, dk, dv errors]) of
    the model against ref_fwd / ref_bwd, the backward reference taking the MODEL's stored out and lse as the GPU tests take the kernel's."""
    mode = MODES["bf16x3"]
    qr, dr = mode.rounded_qkv(qkv), mode.rounded(dout)
    q, k, v = heads(qr, H, 3)
    do = heads(dr, H, 1)[0]
    B, Hh, T, d = q.shape
    scale = d ** -0.5
    s = prod3(q, k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1).float().double()
    P = torch.exp(s - lse[..., None])
    o = round_parts(prod3(P, v), "bf16x3")
    dS = P * (prod3(do, v.transpose(-1, -2)) - (do * o).sum(-1, keepdim=True))
    dq, dk, dv = scale * prod3(dS, k), scale * prod3(dS.transpose(-1, -2), q), prod3(P.transpose(-1, -2), do)
    dqkv = round_parts(torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * Hh * d), "bf16x3")
    out = merge(o)
    o_ref, l_ref = ref_fwd(qr, H)
    g_ref, _ = ref_bwd(qr, out, lse, dr, H)
    return scale_err(out, o_ref), scale_err(lse, l_ref), dqkv_errs(dqkv, g_ref, B, T)
