"""GPU parity of the two precision modes added in round 2, through the C ABI:

  'bf16x3' (MFVIT_BF16X3, split bf16): every MFMA operand is hi + lo (16 mantissa bits), every product three bf16 MFMAs.  It is the
            mode that has to meet BASELINE.json's gate ON the bf16 matrix core: logits within 1e-3 relative of the f32 CPU path and
            bit-exact argmax (the reference's CA finetune is fp32, MAIN_CA:862-882).  Single ops are asserted at 5e-5 of the output
            scale against float64 math on the same (hi + lo) inputs; the encoder / CA step at 1e-3 against the CPU oracle.
  'fp16'   (MFVIT_F16): the reference's autocast arithmetic for pretraining (MAIN_MOCO:349,533): one fp16 rounding of each
            operand / output (2^-11), asserted at 1.5e-3 per op.
"""
import importlib
import os

import pytest
import torch

from conftest import rng_tensor
from oracle import ref_fusion, ref_vit

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_precision.txt")
FUS_MOD = ("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
           "changemodelinputlocation_std002_sum")
SPLIT_TOL = 5e-5
F16_TOL = 1.5e-3


def dev():
    return torch.device("cuda:0")


def log(msg):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")


def rel_err(got, ref):
    ref = ref.double().cpu()
    got = got.double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


ELEM_FLOOR = 0.05      # elementwise-relative checks: |ref| is floored at this fraction of the tensor's largest |ref|


def elem_rel_err(got, ref, floor_frac=ELEM_FLOOR):
    """ELEMENTWISE relative error max_i |got_i - ref_i| / max(|ref_i|, floor), floor = floor_frac x max|ref| (an element closer to zero than the
    floor is judged against the floor: relative error of a number that cancels to ~0 is not defined by any float32 implementation either).
    Returns (error, fraction of elements above the floor).  The scale-relative norm rel_err() is this with floor_frac = 1."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    floor = floor_frac * ref.abs().max().clamp_min(1e-30)
    return float(((got - ref).abs() / ref.abs().clamp_min(floor)).max()), float((ref.abs() >= floor).double().mean())


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


class Mode:
    """How a logical f32 tensor travels to / from the kernels in one precision mode."""

    def __init__(self, name):
        self.name = name
        self.split = name == "bf16x3"
        self.tol = SPLIT_TOL if self.split else F16_TOL

    def pack(self, x):
        from mfvit import ops
        return ops.split_pack(x).to(dev()) if self.split else x.to(torch.float16).to(dev())

    def rounded(self, x):
        """The value the kernel actually sees (float64)."""
        from mfvit import ops
        return ops.split_unpack(ops.split_pack(x)).double() if self.split else x.to(torch.float16).double()

    def unpack(self, y):
        from mfvit import ops
        return ops.split_unpack(y.cpu()) if self.split else y.float().cpu()

    # the qkv operand of the attention core (its own format in the X3F16 mode below)
    def pack_qkv(self, x):
        return self.pack(x)

    def rounded_qkv(self, x):
        return self.rounded(x)


MODES = [Mode("bf16x3"), Mode("fp16")]
IDS = [m.name for m in MODES]


def test_split_pack_layout_and_precision():
    """The torch restatement of the I32 split layout (tests' packer) against its definition, and what it buys: 2^-17 relative."""
    from mfvit import ops
    x = rnd((3, 64), 1)
    s = ops.split_pack(x)
    assert s.shape == (3, 128) and s.dtype == torch.bfloat16
    hi = x.to(torch.bfloat16)
    assert torch.equal(s[:, 0:32], hi[:, 0:32]) and torch.equal(s[:, 64:96], hi[:, 32:64])
    assert torch.equal(s[:, 32:64], (x - hi.float())[:, 0:32].to(torch.bfloat16))
    back = ops.split_unpack(s)
    assert float(((back - x).abs() / x.abs().clamp_min(1e-20)).max()) < 2.0 ** -15
    # cast_transpose writes the same layout (weight shadows)
    w = rnd((384, 1152), 2).to(dev())
    d, dt = ops.cast_transpose(w, torch.bfloat16, split=True)
    assert torch.equal(d.cpu(), ops.split_pack(w.cpu())) and torch.equal(dt.cpu(), ops.split_pack(w.cpu().t().contiguous()))


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("M,N,K", [(300, 384, 384), (128, 1152, 384), (197 * 3, 1536, 384), (64, 384, 1536), (197 * 128, 1152, 384)])
def test_linear_fwd(mode, M, N, K):
    from mfvit import ops
    x, w, b = rnd((M, K), 1), rnd((N, K), 2, 0.05), rnd((N,), 3)
    ref = mode.rounded(x) @ mode.rounded(w).t() + b.double()
    y = ops.linear_fwd(mode.pack(x), mode.pack(w), b.to(dev()), split=mode.split)
    e = rel_err(mode.unpack(y), ref)
    dact, act = ops.linear_fwd(mode.pack(x), mode.pack(w), b.to(dev()), gelu=True, split=mode.split)
    rg = ref.clone().requires_grad_(True)
    torch.nn.functional.gelu(rg).sum().backward()
    # gelu' is kept as plain fp16 in both modes (split tensors: it only ever multiplies a gradient; include/mfvit.h)
    assert dact.dtype == torch.float16 and tuple(dact.shape) == (M, N)
    e1, e2 = rel_err(dact.float().cpu(), rg.grad), rel_err(mode.unpack(act), torch.nn.functional.gelu(ref))
    log(f"linear_fwd[{mode.name},{M},{N},{K}] {e:.2e} gelu' {e1:.2e} gelu {e2:.2e}")
    assert e < mode.tol and e1 < F16_TOL and e2 < mode.tol
    none, act2 = ops.linear_fwd(mode.pack(x), mode.pack(w), b.to(dev()), gelu=True, split=mode.split, want_grad=False)     # no-grad forward
    assert none is None and rel_err(mode.unpack(act2), torch.nn.functional.gelu(ref)) < mode.tol


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("M,N,K", [(777, 256, 384), (100, 384, 1536), (31, 128, 128), (197 * 64, 1152, 384), (197 * 33 + 5, 384, 1536),
                                   (4099, 128, 128), (197 * 128, 1536, 384), (197 * 16, 1152, 384), (2048 + 37, 384, 1536)])
def test_linear_wgrad(mode, M, N, K):
    from mfvit import ops
    dy, x = rnd((M, N), 4), rnd((M, K), 5)
    ref = mode.rounded(dy).t() @ mode.rounded(x)
    dw = ops.linear_wgrad(mode.pack(dy), mode.pack(x), split=mode.split)
    e = rel_err(dw, ref)
    log(f"linear_wgrad[{mode.name},{M},{N},{K}] {e:.2e}")
    assert e < (SPLIT_TOL if mode.split else 1e-4)      # f32 output: only the accumulation order differs
    dw2 = ops.linear_wgrad(mode.pack(dy), mode.pack(x), out=dw.clone(), split=mode.split)
    assert rel_err(dw2, 2 * ref) < (SPLIT_TOL if mode.split else 1e-4)


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("M,K", [(200, 384), (197 * 2, 1536), (64, 768), (197 * 128, 384), (16384 + 77, 1536)])   # > 16,384 rows: two workgroups per CU
def test_linear_res_ln_fwd(mode, M, K):
    from mfvit import ops
    a, w = rnd((M, K), 6), rnd((384, K), 7, 0.05)
    bias, res = rnd((384,), 8), rnd((M, 384), 9)
    gamma, beta = 1 + 0.1 * rnd((384,), 10), rnd((384,), 11, 0.1)
    x_out, y, mean, rstd = ops.linear_res_ln_fwd(mode.pack(a), mode.pack(w), *(t.to(dev()) for t in (bias, res, gamma, beta)), 1e-6,
                                                 split=mode.split)
    xr = mode.rounded(a) @ mode.rounded(w).t() + bias.double() + res.double()
    yr = torch.nn.functional.layer_norm(xr, (384,), gamma.double(), beta.double(), 1e-6)
    es = [rel_err(x_out, xr), rel_err(mode.unpack(y), yr), rel_err(mean, xr.mean(1)), rel_err(rstd, 1 / torch.sqrt(xr.var(1, unbiased=False) + 1e-6))]
    log(f"linear_res_ln_fwd[{mode.name},{M},{K}] {max(es):.2e}")
    assert es[0] < 3e-5 and es[1] < mode.tol and es[2] < 1e-4 and es[3] < 1e-4


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("M,K", [(200, 1152), (197 * 2, 1536), (197 * 65, 1152), (197 * 84 + 13, 1536), (16384 + 64 + 1, 1152)])   # the last two: > 16,384 rows
def test_linear_dgrad_ln_bwd(mode, M, K):
    from mfvit import ops
    dy, wt = rnd((M, K), 12), rnd((384, K), 13, 0.05)
    x, dres = rnd((M, 384), 14), rnd((M, 384), 15)
    gamma = 1 + 0.1 * rnd((384,), 16)
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    bd = torch.zeros(384, dtype=torch.float64, requires_grad=True)
    yln = torch.nn.functional.layer_norm(xd, (384,), gd, bd, 1e-6)
    yln.backward(mode.rounded(dy) @ mode.rounded(wt).t())
    dx_ref = xd.grad + dres.double()
    mean = x.double().mean(1)
    rstd = 1 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-6)
    dx, dx_t, dgamma, dbeta, dcol = ops.linear_dgrad_ln_bwd(mode.pack(dy), mode.pack(wt), x.to(dev()), mean.float().to(dev()),
                                                           rstd.float().to(dev()), gamma.to(dev()), dres.to(dev()), split=mode.split)
    es = [rel_err(dx, dx_ref), rel_err(mode.unpack(dx_t), dx_ref), rel_err(dgamma, gd.grad), rel_err(dbeta, bd.grad), rel_err(dcol, dx_ref.sum(0))]
    log(f"linear_dgrad_ln_bwd[{mode.name},{M},{K}] {max(es):.2e}")
    assert es[0] < 5e-5 and es[1] < mode.tol and es[2] < 1e-4 and es[3] < 1e-4 and es[4] < 1e-4
    if M > 16384:     # the same without the residual-gradient input and without the operand-type copy
        dx2, none, dg2, db2, dc2 = ops.linear_dgrad_ln_bwd(mode.pack(dy), mode.pack(wt), x.to(dev()), mean.float().to(dev()),
                                                           rstd.float().to(dev()), gamma.to(dev()), None, want_copy=False, split=mode.split)
        assert none is None and rel_err(dx2, xd.grad) < 5e-5 and rel_err(dg2, gd.grad) < 1e-4 and rel_err(dc2, xd.grad.sum(0)) < 1e-4


def _attn_ref(qkv, heads):
    B, T, D3 = qkv.shape
    D = D3 // 3
    d = D // heads
    q, k, v = qkv.reshape(B, T, 3, heads, d).permute(2, 0, 3, 1, 4)
    a = (q @ k.transpose(-2, -1)) * d ** -0.5
    lse = torch.logsumexp(a, dim=-1)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(B, T, D)
    return o, lse


class Bf16Mode(Mode):
    def __init__(self):
        self.name, self.split, self.tol = "bf16", False, 8e-3

    def pack(self, x):
        return x.to(torch.bfloat16).to(dev())

    def rounded(self, x):
        return x.to(torch.bfloat16).double()


class X3F16Mode(Mode):
    """What the encoder runs in bf16x3 mode (round 5): qkv in SPLIT FP16 (dtype tag MFVIT_X3F16), out / dout / dqkv split bf16.  The forward
    splits P into two fp16 parts (f32-grade); the backward feeds P and dS as ONE fp16 part (11 bits: gradients at the level of the
    MLP's saved fp16 activation derivative)."""

    def __init__(self):
        super().__init__("bf16x3")
        self.name = "x3f16"

    def pack_qkv(self, x):
        from mfvit import ops
        return ops.split_pack_f16(x).to(dev())

    def rounded_qkv(self, x):
        x = x.float()
        hi = x.to(torch.float16)
        return hi.double() + (x - hi.float()).to(torch.float16).double()


ATT_MODES = MODES + [Bf16Mode(), X3F16Mode()]


def bwd_tol(mode):
    # backward: D = rowsum(dO o O) uses the rounded O; P / dS re-rounded (x3f16: to ONE fp16 part: 2^-11 per element, measured 3e-4 .. 5e-4)
    return {"bf16x3": 2e-4, "x3f16": 1e-3, "fp16": 4e-3}.get(mode.name, 2e-2)


@pytest.mark.parametrize("mode", ATT_MODES, ids=[m.name for m in ATT_MODES])
@pytest.mark.parametrize("B,T,H", [(2, 197, 12), (3, 50, 12), (1, 256, 12),      # whole-head-in-LDS kernels (attention_mfma.hip)
                                   (1, 577, 12),                                 # 384^2 inputs: split bf16 streams (attention_tiled.hip)
                                   (2, 394, 4), (1, 130, 4),                     # TransFuser-GPT heads: 4 x 96 over 394 joint tokens (tiled)
                                   (2, 197, 6), (1, 1200, 12),                   # head_dim 64; a sequence beyond the LDS images (tiled)
                                   (45, 197, 12)])                               # B * H = 540 > 2 x #CUs, not a multiple of it: the PERSISTENT
                                                                                 # multi-pair loops of both directions with a ragged tail
def test_attention_fwd_bwd(mode, B, T, H):
    from mfvit import ops
    D = 384
    qkv, dout = rnd((B, T, 3 * D), 17), rnd((B, T, D), 18)
    # split layout of qkv: per token [3][H][head_dim / 32 groups of hi x 32 | lo x 32] = the I32 layout of the 1152 logical columns
    if mode.name == "x3f16" and ops.attention_qkv_dtype(2, T, D // H) != 4:
        pytest.skip("split-fp16 qkv exists for the whole-head kernels only (head_dim 32, T <= 224)")
    qd = mode.rounded_qkv(qkv).requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qd, H)
    out, lse = ops.attention_fwd(mode.pack_qkv(qkv), H, split=mode.split)
    e_o, e_l = rel_err(mode.unpack(out), o_ref), rel_err(lse, lse_ref)
    # the backward sees the rounded upstream gradient (what the previous kernel would hand it) and the stored (rounded) output
    o_ref.backward(mode.rounded(dout))
    dqkv, dbias = ops.attention_bwd(mode.pack_qkv(qkv), out, mode.pack(dout), lse, H, split=mode.split)
    e_d, e_b = rel_err(mode.unpack(dqkv), qd.grad), rel_err(dbias, qd.grad.sum((0, 1)))
    log(f"attention[{mode.name},B={B},T={T},H={H}] out {e_o:.2e} lse {e_l:.2e} dqkv {e_d:.2e} dbias {e_b:.2e}")
    t = bwd_tol(mode)
    assert e_o < mode.tol and e_l < 1e-5 and e_d < t and e_b < t


@pytest.mark.parametrize("mode", ATT_MODES, ids=[m.name for m in ATT_MODES])
def test_attention_two_phase_backward_behind_its_switch(monkeypatch, mode):
    """The persistent two-phase backward with register prefetch (csrc/attention_mfma.hip; MFVIT_ATTN_BWD_SP=0: what sequence lengths other than
    7 row tiles run) against float64 at B * H = 540, T = 197, where the default is the single-pass kernel (test_attention_fwd_bwd[45-197-12],
    test_attention_single_pass_backward_tile_edges)."""
    from mfvit import ops
    monkeypatch.setenv("MFVIT_ATTN_BWD_SP", "0")          # (tests/conftest.py sets MFVIT_AB_LIVE=1: switches are read at every launch)
    B, T, H, D = 45, 197, 12, 384
    qkv, dout = rnd((B, T, 3 * D), 27), rnd((B, T, D), 28)
    qd = mode.rounded_qkv(qkv).requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qd, H)
    out, lse = ops.attention_fwd(mode.pack_qkv(qkv), H, split=mode.split)
    e_o, e_l = rel_err(mode.unpack(out), o_ref), rel_err(lse, lse_ref)
    o_ref.backward(mode.rounded(dout))
    dqkv, dbias = ops.attention_bwd(mode.pack_qkv(qkv), out, mode.pack(dout), lse, H, split=mode.split)
    e_d, e_b = rel_err(mode.unpack(dqkv), qd.grad), rel_err(dbias, qd.grad.sum((0, 1)))
    log(f"attention persistent kernels[{mode.name},B={B}] out {e_o:.2e} lse {e_l:.2e} dqkv {e_d:.2e} dbias {e_b:.2e}")
    t = bwd_tol(mode)
    assert e_o < mode.tol and e_l < 1e-5 and e_d < t and e_b < t


@pytest.mark.parametrize("mode", ATT_MODES, ids=[m.name for m in ATT_MODES])
@pytest.mark.parametrize("T", [193, 208, 209, 224])
def test_attention_single_pass_backward_tile_edges(mode, T):
    """The single-pass backward (attn_bwd_sp_kernel: seven row tiles, B * H >= 2 x #CUs) at the edges of its last tile: one valid row in
    it (193), exactly its first / just into its second 16-row half (208 / 209), no padding at all (224); 43 x 12 = 516 pairs, so
    workgroups own two or three pairs (first, middle and last pair of a persistent loop).  dq / dk / dv separately against float64."""
    from mfvit import ops
    B, H, D = 43, 12, 384
    qkv, dout = rnd((B, T, 3 * D), 31 + T), rnd((B, T, D), 32 + T)
    qd = mode.rounded_qkv(qkv).requires_grad_(True)
    o_ref, _ = _attn_ref(qd, H)
    out, lse = ops.attention_fwd(mode.pack_qkv(qkv), H, split=mode.split)
    o_ref.backward(mode.rounded(dout))
    dqkv, dbias = ops.attention_bwd(mode.pack_qkv(qkv), out, mode.pack(dout), lse, H, split=mode.split)
    g, r = mode.unpack(dqkv).view(B, T, 3, D), qd.grad.view(B, T, 3, D)
    es = [rel_err(g[:, :, i], r[:, :, i]) for i in range(3)]
    log(f"attention single-pass backward[{mode.name},T={T}] dq {es[0]:.2e} dk {es[1]:.2e} dv {es[2]:.2e} dbias {rel_err(dbias, qd.grad.sum((0, 1))):.2e}")
    assert max(es) < bwd_tol(mode) and torch.isfinite(dqkv.float()).all()


@pytest.mark.parametrize("mode", ATT_MODES, ids=[m.name for m in ATT_MODES])
@pytest.mark.parametrize("T", [129, 160, 161, 192])
def test_attention_persistent_forward_row_tile_counts(monkeypatch, mode, T):
    """The persistent producer-wave forward (attn_fwd_pp_kernel) at FIVE and SIX row tiles per pair (T = 129 / 160: 5, 161 / 192: 6 - idle
    computing waves, the `t + 1 < nt` tail of the step sequence, the image / pad geometry at T % 32 == 0 and at one row into a tile), with
    43 x 12 = 516 pairs so that it is the kernel that runs for the split types (bf16 / fp16 run the per-pair kernel at the same
    shapes).  Output and log-sum-exp against float64; the backward at these lengths is the two-phase kernel."""
    from mfvit import ops
    B, H, D = 43, 12, 384
    qkv, dout = rnd((B, T, 3 * D), 41 + T), rnd((B, T, D), 42 + T)
    qd = mode.rounded_qkv(qkv).requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qd, H)
    out, lse = ops.attention_fwd(mode.pack_qkv(qkv), H, split=mode.split)
    e_o, e_l = rel_err(mode.unpack(out), o_ref), rel_err(lse, lse_ref)
    o_ref.backward(mode.rounded(dout))
    dqkv, _ = ops.attention_bwd(mode.pack_qkv(qkv), out, mode.pack(dout), lse, H, want_dbias=False, split=mode.split)
    e_d = rel_err(mode.unpack(dqkv), qd.grad)
    log(f"attention persistent forward[{mode.name},T={T}] out {e_o:.2e} lse {e_l:.2e} dqkv {e_d:.2e}")
    assert e_o < mode.tol and e_l < 1e-5 and e_d < bwd_tol(mode) and torch.isfinite(out.float()).all()


def test_attention_split_fp16_part_counts():
    """The split-fp16 attention with P in two fp16 parts in the forward and dS / P in ONE in the backward (11 bits), with a gradient-scale dO
    (1e-4: below fp16's normal range - the kernels scale it per (image, head)), at the bench kernels' shape class (B * H = 540: persistent forward,
    single-pass backward) and on the per-pair kernels (B = 2)."""
    from mfvit import ops
    mode = X3F16Mode()
    H, D, T = 12, 384, 197
    for B in (45, 2):
        qkv, dout = rnd((B, T, 3 * D), 51 + B), rnd((B, T, D), 52 + B, 1e-4)       # gradient-scale dO: the kernels scale it into fp16's range
        qd = mode.rounded_qkv(qkv).requires_grad_(True)
        o_ref, lse_ref = _attn_ref(qd, H)
        out, lse = ops.attention_fwd(mode.pack_qkv(qkv), H, split=True)
        o_ref.backward(mode.rounded(dout))
        dqkv, dbias = ops.attention_bwd(mode.pack_qkv(qkv), out, mode.pack(dout), lse, H, split=True)
        e_o, e_d = rel_err(mode.unpack(out), o_ref), rel_err(mode.unpack(dqkv), qd.grad)
        log(f"attention split fp16, parts fwd 2 bwd 1 [B={B}] out {e_o:.2e} dqkv {e_d:.2e} dbias {rel_err(dbias, qd.grad.sum((0, 1))):.2e}")
        assert e_o < SPLIT_TOL and e_d < 1e-3


def test_layernorm_rows_split_and_f16():
    from mfvit import ops
    rows, N = 333, 384
    x, dy, dres = rnd((rows, N), 19, 2.0), rnd((rows, N), 20), rnd((rows, N), 21)
    gamma, beta = 1 + 0.1 * rnd((N,), 22), rnd((N,), 23, 0.1)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xd, (N,), gd, bd, 1e-5)
    yr.backward(dy.double())
    ref = xd.grad + dres.double()
    for mode in MODES:
        dt = torch.bfloat16 if mode.split else torch.float16
        y, mean, rstd = ops.layernorm_fwd(x.to(dev()), gamma.to(dev()), beta.to(dev()), 1e-5, out_dtype=dt, split=mode.split)
        assert rel_err(mode.unpack(y), yr) < mode.tol
        dx, dx_t, dgamma, dbeta, dcol = ops.layernorm_bwd(dy.to(dev()), x.to(dev()), mean, rstd, gamma.to(dev()), dres.to(dev()),
                                                         copy_dtype=dt, split=mode.split)
        assert rel_err(dx, ref) < 1e-5 and rel_err(mode.unpack(dx_t), ref) < mode.tol


# ------------------------------------------------------------------------------------------------ encoder / CA step
def build(precision, seed, depth=12, num_classes=3, img=224, **kw):
    import vits
    m = vits.vit_small(num_classes=num_classes, depth=depth, precision=precision, img_size=img, **kw)
    p = ref_vit.seeded_params(seed, num_classes=num_classes, depth=depth, img_size=img)
    m.load_state_dict(p, strict=True)
    return m.to("cuda:0"), p


@pytest.mark.parametrize("B,img", [(2, 224), (3, 64)])
def test_bf16x3_encoder_meets_the_1e3_gate(B, img):
    """12 blocks, split bf16: features and logits within 1e-3 relative of the f32 CPU oracle, argmax bit-exact (north star)."""
    m, p = build("bf16x3", 501, img=img)
    x = rng_tensor(502, (B, 3, img, img))
    with torch.no_grad():
        ref_f = ref_vit.features3d(p, x)
        ref_l = ref_vit.head_linear(p, ref_f[:, 0])
        f = m.features3D(x.to("cuda:0"))
        logits = m(x.to("cuda:0"))
    e_f, e_l = rel_err(f, ref_f), rel_err(logits, ref_l)
    log(f"encoder[bf16x3,B={B},img={img}] features {e_f:.2e} logits {e_l:.2e}")
    assert e_f < 1e-3 and e_l < 1e-3
    assert logits.argmax(1).cpu().tolist() == ref_l.argmax(1).tolist()


@pytest.mark.parametrize("precision,tol", [("bf16x3", 2e-3), ("fp16", 2e-2)])
@pytest.mark.parametrize("stop_grad_conv1", [False, True])
def test_backward_all_parameters(precision, tol, stop_grad_conv1):
    B, depth = 2, 3
    m, p = build(precision, 511, depth=depth, stop_grad_conv1=stop_grad_conv1)
    x = rng_tensor(512, (B, 3, 224, 224))
    r = rng_tensor(513, (B, 197, 384))
    rl = rng_tensor(514, (B, 3))
    pd = {k: v.double().requires_grad_(k != "pos_embed") for k, v in p.items()}
    f_ref = ref_vit.features3d(pd, x.double())
    loss_ref = (f_ref * r.double()).sum() + (ref_vit.head_linear(pd, f_ref[:, 0]) * rl.double()).sum()
    loss_ref.backward()
    xg = x.to("cuda:0")
    f = m.features3D(xg)
    loss = (f * r.to("cuda:0")).sum() + (m(xg) * rl.to("cuda:0")).sum()
    loss.backward()
    worst = ("", 0.0)
    for name, prm in m.named_parameters():
        if name == "pos_embed" or (stop_grad_conv1 and name.startswith("patch_embed")):
            assert prm.grad is None
            continue
        e = rel_err(prm.grad, pd[name].grad)
        if e > worst[1]:
            worst = (name, e)
        assert e < tol, (name, e)
    log(f"backward[{precision},stop_grad_conv1={stop_grad_conv1}] worst {worst[0]} err={worst[1]:.2e}")


@pytest.mark.parametrize("precision,tol_f,tol_g", [("bf16x3", 1e-4, 2e-3), ("fp16", 6e-3, 2e-2), ("bf16", 4e-2, 8e-2)])
def test_backward_on_the_size_gated_kernels_against_the_oracle(precision, tol_f, tol_g):
    """B = 24 images = 4,728 token rows (>= 4,096) and B * H = 288 (image, head) pairs (> #CUs): the encoder takes the kernels the TIMED step
    runs - the tall-tile row kernels of csrc/gemm_rowp.hip, the LDS-DMA weight gradients with dWproj riding along with dWqkv
    (`gemm_tn_glds_pair`), the persistent multi-pair attention loops - and every parameter gradient is compared with the float64 CPU
    oracle (depth 2 keeps it in seconds).  The B <= 3 oracle tests run the small-M kernels only."""
    B, depth = 24, 2
    m, p = build(precision, 521, depth=depth)
    x = rng_tensor(522, (B, 3, 224, 224))
    r = rng_tensor(523, (B, 197, 384))
    pd = {k: v.double().requires_grad_(k != "pos_embed") for k, v in p.items()}
    f_ref = ref_vit.features3d(pd, x.double())
    (f_ref * r.double()).sum().backward()
    f = m.features3D(x.to("cuda:0"))
    (f * r.to("cuda:0")).sum().backward()
    e_f = rel_err(f, f_ref)
    worst = ("", 0.0)
    for name, prm in m.named_parameters():
        if name == "pos_embed" or name.startswith("head"):
            continue
        e = rel_err(prm.grad, pd[name].grad)
        if e > worst[1]:
            worst = (name, e)
        assert e < tol_g, (name, e)
    log(f"size-gated backward[{precision}, B={B}, depth {depth}] features {e_f:.2e} worst grad {worst[0]} {worst[1]:.2e}")
    assert e_f < tol_f


def test_fp16_encoder_forward():
    m, p = build("fp16", 501)
    x = rng_tensor(502, (2, 3, 224, 224))
    with torch.no_grad():
        ref_f = ref_vit.features3d(p, x)
        f = m.features3D(x.to("cuda:0"))
    e = rel_err(f, ref_f)
    log(f"encoder[fp16,B=2] features {e:.2e}")
    assert e < 6e-3      # 2^-11 roundings through 12 blocks (bf16: 4.7e-3 .. 6.9e-3 at 2^-8)


def test_bf16x3_ca_step_meets_the_1e3_gate():
    """Two-stream CA train step (Fus_CrossViT forward, output sum, CE, backward) in the default headline precision against the CPU
    oracle: logits 1e-3 + bit-exact argmax, loss, and fusion / backbone gradients at 2e-3."""
    import vits_returnftrs as vits
    from mfvit.losses import cross_entropy
    fus = importlib.import_module(FUS_MOD)
    depth, B = 12, 2
    vit_p = [ref_vit.seeded_params(7 + i, num_classes=3, depth=depth) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(9)
    backs = []
    for p in vit_p:
        m = vits.vit_small(num_classes=3, depth=depth, precision="bf16x3")
        m.load_state_dict(p)
        backs.append(m.to("cuda:0"))
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    model = model.to("cuda:0")
    x, xe = rng_tensor(81, (B, 3, 224, 224)), rng_tensor(82, (B, 3, 224, 224))
    y = torch.tensor([1, 2])
    fused, x_c, x_e = model(backs[0], backs[1], x.to("cuda:0"), xe.to("cuda:0"))
    out = fused + x_c + x_e
    loss, preds = cross_entropy(out, y.to("cuda:0"))
    loss.backward()
    fpd = {k: v.clone().requires_grad_(True) for k, v in fus_p.items()}
    vpd = [{k: v.clone().requires_grad_(k != "pos_embed") for k, v in p.items()} for p in vit_p]
    r_out, r_preds, r_loss, _ = ref_fusion.ca_step(fpd, vpd[0], vpd[1], x, xe, y)
    r_loss.backward()
    e_out = rel_err(out, r_out)
    k = "multi_scale_transformers.0.cross_attn_layers.0.0.fn.wk.weight"
    e_f = rel_err(dict(model.named_parameters())[k].grad, fpd[k].grad)
    e_b = max(rel_err(backs[i].blocks[j].attn.qkv.weight.grad, vpd[i][f"blocks.{j}.attn.qkv.weight"].grad) for i in (0, 1) for j in (0, 11))
    e_el, above = elem_rel_err(out, r_out)
    log(f"CA step[bf16x3, depth 12] logits {e_out:.2e} (elementwise, |ref| floored at {ELEM_FLOOR} max|ref|: {e_el:.2e}, {100 * above:.0f} % of the logits above the floor) "
        f"fusion-grad {e_f:.2e} backbone-grad {e_b:.2e} loss {float(loss):.6f} vs {float(r_loss):.6f}")
    # forward: the north star's 1e-3, scale-relative AND elementwise; gradients: bf16x3 carries fp16-grade parts in the backward (gelu', P / dS: measured
    # 2.2e-4 ... 5.7e-4) - asserted at 1e-3 since round 6 (2e-3 before)
    assert e_out < 1e-3 and e_el < 1e-3 and e_f < 1e-3 and e_b < 1e-3
    assert preds.cpu().tolist() == r_preds.tolist()
    assert abs(float(loss) - float(r_loss)) < 1e-4 * max(1.0, abs(float(r_loss)))


def test_bf16x3_ca_step_at_the_bench_shape_against_the_oracle():
    """The SAME step at the shape bench.py times (BASELINE configs[2]: 128 pairs, depth 12, M = 25,216 token rows per encoder - every
    size-gated kernel of the timed step: tall row tiles with 7 fragments, the paired weight gradient, the persistent attention forward
    and the single-pass backward at 1,536 (image, head) pairs) against the CPU oracle's forward AND backward on the same weights and
    inputs: all 128 logit rows, argmax, loss, and the qkv / fc2 / patch-embedding weight gradients of both backbones plus a fusion
    gradient."""
    import vits_returnftrs as vits
    from mfvit.losses import cross_entropy
    fus = importlib.import_module(FUS_MOD)
    depth, B = 12, 128
    vit_p = [ref_vit.seeded_params(37 + i, num_classes=3, depth=depth) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(39)
    backs = []
    for p in vit_p:
        m = vits.vit_small(num_classes=3, depth=depth, precision="bf16x3")
        m.load_state_dict(p)
        backs.append(m.to("cuda:0"))
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    model = model.to("cuda:0")
    x, xe = rng_tensor(83, (B, 3, 224, 224)), rng_tensor(84, (B, 3, 224, 224))
    y = torch.arange(B) % 3
    fused, x_c, x_e = model(backs[0], backs[1], x.to("cuda:0"), xe.to("cuda:0"))
    out = fused + x_c + x_e
    loss, preds = cross_entropy(out, y.to("cuda:0"))
    loss.backward()
    fpd = {k: v.clone().requires_grad_(True) for k, v in fus_p.items()}
    vpd = [{k: v.clone().requires_grad_(k != "pos_embed") for k, v in p.items()} for p in vit_p]
    r_out, r_preds, r_loss, _ = ref_fusion.ca_step(fpd, vpd[0], vpd[1], x, xe, y)
    r_loss.backward()
    e_out = rel_err(out, r_out)
    k = "multi_scale_transformers.0.cross_attn_layers.0.0.fn.wk.weight"
    e_f = rel_err(dict(model.named_parameters())[k].grad, fpd[k].grad)
    e_b = 0.0
    for i in (0, 1):
        for j in (0, 5, 11):
            e_b = max(e_b, rel_err(backs[i].blocks[j].attn.qkv.weight.grad, vpd[i][f"blocks.{j}.attn.qkv.weight"].grad),
                      rel_err(backs[i].blocks[j].mlp.fc2.weight.grad, vpd[i][f"blocks.{j}.mlp.fc2.weight"].grad),
                      rel_err(backs[i].blocks[j].norm1.weight.grad, vpd[i][f"blocks.{j}.norm1.weight"].grad))
        e_b = max(e_b, rel_err(backs[i].patch_embed.proj.weight.grad, vpd[i]["patch_embed.proj.weight"].grad))
    log(f"CA step[bf16x3, depth 12, B = {B}: the bench shape] logits {e_out:.2e} fusion-grad {e_f:.2e} backbone-grads {e_b:.2e} "
        f"loss {float(loss):.6f} vs {float(r_loss):.6f}")
    e_el, above = elem_rel_err(out, r_out)
    log(f"  the same {B} x 3 logits ELEMENTWISE (|ref| floored at {ELEM_FLOOR} max|ref|): {e_el:.2e}, {100 * above:.0f} % of them above the floor")
    assert e_out < 1e-3 and e_el < 1e-3 and e_f < 1e-3 and e_b < 1e-3
    assert preds.cpu().tolist() == r_preds.tolist()
    assert abs(float(loss) - float(r_loss)) < 1e-4 * max(1.0, abs(float(r_loss)))


def test_grad_scaler_semantics():
    """mfvit.amp.GradScaler against torch's documented behaviour (MAIN_MOCO:546-548): unscale + step on clean gradients, skip +
    backoff on an overflow, growth after `growth_interval` clean steps, state_dict keys."""
    from mfvit.amp import GradScaler
    from mfvit.optim import SGD
    w = torch.nn.Parameter(torch.ones(70000, device="cuda:0"))
    opt = SGD([w], lr=0.5, momentum=0.0)
    sc = GradScaler(init_scale=1024.0, growth_interval=2)
    assert float(sc.scale(torch.tensor(2.0, device="cuda:0"))) == 2048.0
    w.grad = torch.full_like(w, 1024.0 * 0.25)          # = scale * true gradient 0.25
    sc.step(opt); sc.update()
    assert torch.allclose(w.detach(), torch.full_like(w, 1.0 - 0.5 * 0.25)) and sc.get_scale() == 1024.0
    w.grad = torch.full_like(w, 1024.0 * 0.25)
    w.grad[69999] = float("inf")                          # overflow in the last chunk: the step is skipped, the scale halves
    before = w.detach().clone()
    assert sc.step(opt) is None
    sc.update()
    assert torch.equal(w.detach(), before) and sc.get_scale() == 512.0
    for _ in range(2):                                    # two clean steps -> growth
        w.grad = torch.full_like(w, 512.0 * 0.1)
        sc.step(opt); sc.update()
    assert sc.get_scale() == 1024.0
    assert set(sc.state_dict()) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    sc2 = GradScaler()
    sc2.load_state_dict(sc.state_dict())
    assert sc2.get_scale() == 1024.0
    w.grad = torch.full_like(w, float("nan"))
    assert sc.step(opt) is None


@pytest.mark.parametrize("precision,tol", [("fp16", 2e-2), ("bf16x3", 1e-3)])
def test_two_stream_384_ca_step(precision, tol):
    """BASELINE configs[4] shape: two-stream MF-ViT CA step at 384 x 384 (577 tokens per stream) in the config's own arithmetic (fp16)
    and in the f32-grade default (split bf16: 577 tokens are beyond the whole-head LDS images, so the streaming attention kernels of
    csrc/attention_tiled.hip run).  Forward + backward against the CPU oracle (depth 2 keeps the oracle in seconds)."""
    import vits_returnftrs as vits
    from mfvit.losses import cross_entropy
    fus = importlib.import_module(FUS_MOD)
    depth, B, img = 2, 2, 384
    vit_p = [ref_vit.seeded_params(17 + i, num_classes=3, depth=depth, img_size=img) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(19)
    backs = []
    for p in vit_p:
        m = vits.vit_small(num_classes=3, depth=depth, precision=precision, img_size=img)
        m.load_state_dict(p)
        backs.append(m.to("cuda:0"))
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    model = model.to("cuda:0")
    x, xe = rng_tensor(91, (B, 3, img, img)), rng_tensor(92, (B, 3, img, img))
    y = torch.tensor([2, 0])
    fused, x_c, x_e = model(backs[0], backs[1], x.to("cuda:0"), xe.to("cuda:0"))
    out = fused + x_c + x_e
    loss, preds = cross_entropy(out, y.to("cuda:0"))
    loss.backward()
    fpd = {k: v.clone().requires_grad_(True) for k, v in fus_p.items()}
    vpd = [{k: v.clone().requires_grad_(k != "pos_embed") for k, v in p.items()} for p in vit_p]
    r_out, r_preds, r_loss, _ = ref_fusion.ca_step(fpd, vpd[0], vpd[1], x, xe, y)
    r_loss.backward()
    e_out = rel_err(out, r_out)
    e_b = max(rel_err(backs[i].blocks[j].attn.qkv.weight.grad, vpd[i][f"blocks.{j}.attn.qkv.weight"].grad) for i in (0, 1) for j in (0, 1))
    log(f"two-stream 384^2 CA step [{precision}]: logits {e_out:.2e} backbone-grad {e_b:.2e} loss {float(loss):.6f} vs {float(r_loss):.6f}")
    assert e_out < tol and e_b < 2 * tol
    if precision == "bf16x3":
        assert preds.cpu().tolist() == r_preds.tolist()


def test_two_stream_384_forward_at_the_configs_own_batch():
    """BASELINE configs[4] at its per-GPU size: depth 12, 32 pairs of 384 x 384 inputs (577 tokens per stream), fp16 - the need-grad forward
    of the train step (the kernels bench.py times for `--img 384 --precision fp16 --batch 32`: streaming attention at B * H = 384 pairs,
    row kernels at M = 18,464) against the CPU oracle on the same weights and inputs; the backward at this shape is covered through the
    sample-independence property (gradient of the batch = sum over its halves) with the oracle-compared B = 2 test above."""
    import vits_returnftrs as vits
    from mfvit.losses import cross_entropy
    fus = importlib.import_module(FUS_MOD)
    depth, B, img = 12, 32, 384
    vit_p = [ref_vit.seeded_params(27 + i, num_classes=3, depth=depth, img_size=img) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(29)
    backs = []
    for p in vit_p:
        m = vits.vit_small(num_classes=3, depth=depth, precision="fp16", img_size=img)
        m.load_state_dict(p)
        backs.append(m.to("cuda:0"))
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    model = model.to("cuda:0")
    x, xe = rng_tensor(93, (B, 3, img, img)), rng_tensor(94, (B, 3, img, img))
    y = torch.arange(B) % 3

    def grads(lo, hi):
        for m in backs:
            for p_ in m.parameters():
                p_.grad = None
        fused, x_c, x_e = model(backs[0], backs[1], x[lo:hi].to("cuda:0"), xe[lo:hi].to("cuda:0"))
        out = fused + x_c + x_e
        loss, _ = cross_entropy(out, y[lo:hi].to("cuda:0"))
        (loss * (hi - lo)).backward()                                   # sum over the samples: additive over sub-batches
        return out.detach(), [backs[i].blocks[j].attn.qkv.weight.grad.clone() for i in (0, 1) for j in (0, 11)]
    out, g_all = grads(0, B)
    with torch.no_grad():
        r_out, r_preds, r_loss, _ = ref_fusion.ca_step(fus_p, vit_p[0], vit_p[1], x, xe, y)
    e_out = rel_err(out, r_out)
    _, g_a = grads(0, B // 2)
    _, g_b = grads(B // 2, B)
    e_add = max(rel_err(ga + gb, g) for ga, gb, g in zip(g_a, g_b, g_all))
    log(f"two-stream 384^2 forward [fp16, depth 12, B = {B}]: logits {e_out:.2e}; grad(batch) vs grad(half) + grad(half) {e_add:.2e}")
    assert e_out < 2e-2 and e_add < 2e-2


@pytest.mark.parametrize("B,T", [(2, 197), (3, 50), (1, 256), (2, 33)])
def test_qkv_projection_in_split_fp16(B, T):
    """mfvit_linear_fwd epilogue 5 (the encoder's qkv projection in bf16x3 mode): y = x W^T + b written as SPLIT FP16 (MFVIT_X3F16), against
    float64 on the same split-bf16 inputs - hi + lo of the stored pair at 2^-21 of the tensor's scale - and straight into the attention core."""
    from mfvit import ops
    mode = X3F16Mode()
    H, D = 12, 384
    x, w, bias = rnd((B, T, D), 31), rnd((3 * D, D), 32, 0.05), rnd((3 * D,), 33, 0.5)
    xr, wr = mode.rounded(x), mode.rounded(w)
    qkv_ref = xr @ wr.t() + bias.double()
    o_ref, lse_ref = _attn_ref(qkv_ref, H)
    qkv = ops.linear_fwd(mode.pack(x).reshape(B * T, -1), mode.pack(w), bias.to(dev()), split=True, qkv_f16=True).reshape(B, T, -1)
    assert qkv.dtype == torch.float16 and ops.attention_qkv_dtype(2, T, D // H) == (4 if T <= 224 else 2)
    if T > 224:
        return
    g = qkv.cpu().reshape(B, T, -1, 2, 32).double()
    e_q = rel_err((g[..., 0, :] + g[..., 1, :]).reshape(B, T, 3 * D), qkv_ref)
    out, lse = ops.attention_fwd(qkv, H, split=True)
    e_o, e_l = rel_err(mode.unpack(out), o_ref), rel_err(lse, lse_ref)
    log(f"qkv projection in split fp16 [B={B},T={T}] qkv {e_q:.2e} out {e_o:.2e} lse {e_l:.2e}")
    assert e_q < 5e-6 and e_o < 2 * SPLIT_TOL and e_l < 1e-5


def test_persistent_forward_attention_is_the_same_bits_from_run_to_run():
    """Round 6: the tile-0 row maximum of attn_fwd_pp_kernel was an inline-asm v_max3 right behind the tile's score MFMAs - no wait states from the compiler,
    accumulator registers read before the last MFMA had written them.  The softmax is correct for ANY reference maximum, so every result stayed inside its
    tolerance, but ~2 % of the rows moved by a rounding from run to run (and a far-off reference could overflow the fp16 probabilities).  Fixed by a
    compiler-visible maximum for tile 0; tools/check_mfma_asm_hazards.py now scans every build.  Here: B x H = 1,152 pairs (the persistent kernel), five runs,
    out and lse bit for bit - in the split-fp16 operand format of the shipped path and in split bf16."""
    from mfvit import ops
    B, T, H, D = 96, 197, 12, 384
    qkv = rnd((B, T, 3 * D), 77)
    for name, pack in (("split fp16", ops.split_pack_f16), ("split bf16", ops.split_pack)):
        q = pack(qkv.to(dev()))
        o0, l0 = ops.attention_fwd(q, H, split=True)
        for _ in range(4):
            o, l = ops.attention_fwd(q, H, split=True)
            assert torch.equal(o.view(torch.int16), o0.view(torch.int16)) and torch.equal(l, l0), name
    log(f"attention persistent forward: out / lse bit-identical over 5 runs (B = {B}, split fp16 and split bf16 qkv)")


@pytest.mark.parametrize("B", [16, 128])
def test_ca_train_step_is_the_same_bits_from_run_to_run(B):
    """Round 6: every sum of the two-stream CA step is taken in a fixed order - forward, loss and all 324 parameter-gradient tensors (two encoders, the
    cross-attention fusion, the four classifier heads) are bit-identical over three runs on the same weights and inputs; Adam is elementwise, so a training run
    on one GPU is reproducible bit for bit.  What used float atomics until this round: the column partials of the row kernels and of the x gelu' tile epilogue,
    the bias sums of the weight-gradient kernels, cls_token / patch-embedding bias (csrc/gemm.hip::colpart_reduce, gemm_tn2.hip, gemm_pp.hip,
    elementwise.hip::colsum_rows) and the small gradients of the fusion (csrc/fusion.hip: per-sample partial rows + one fixed-order reduce).  B = 128 is
    BASELINE configs[2]; B = 16 runs the K-split row kernels and the weight-gradient side stream."""
    import sys
    import bench
    argv, sys.argv = sys.argv, sys.argv[:1]              # (bench.parse reads the command line: defaults only)
    try:
        args = bench.parse()
    finally:
        sys.argv = argv
    args.batch = B
    run = bench.CaRun(args, dev(), 0, "bf16x3", "T")

    def once():
        run.opt.zero_grad(set_to_none=True)
        fused, x_c, x_e = run.model(run.backs[0], run.backs[1], run.x, run.xe)
        out = fused + x_c + x_e
        loss, _ = run._ce(out, run.target)
        loss.backward()
        torch.cuda.synchronize()
        g = [out.detach().clone(), loss.detach().clone()]
        for mod in (run.model, run.backs[0], run.backs[1]):
            g += [p.grad.detach().clone() for p in mod.parameters() if p.grad is not None]
        return g

    once()
    a, b, c = once(), once(), once()
    assert len(a) == 326                                  # logits, loss, 324 gradient tensors
    for i, (x, y, z) in enumerate(zip(a, b, c)):
        assert torch.equal(x, y) and torch.equal(x, z), i
    log(f"CA train step (B = {B}): logits, loss and {len(a) - 2} gradient tensors bit-identical over three runs")
