"""GPU parity of the token-input (GPT) encoder at its token, head and width edges (case table and error measures: tests/gpt_edges_ref.py; the
CPU side: tests/test_gpt_edges_cpu.py).  model/fuseattention.py::GPT -> mfvit/gpt.py -> mfvit_gpt_forward / mfvit_gpt_backward against the
float64 oracle (oracle/ref_gpt.py): head widths 32 / 64 / 96, M = B T from 5 rows up, width 768, all four operand types, both activations,
dropout at the edges, sample independence, and the C ABI's own contract (accumulated dparams, every output row written, argument errors)."""
import types

import pytest
import torch

import gpt_edges_ref as ge
from conftest import rng_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
CASE_PRECISION = [(c.name, p) for c in ge.CASES for p in c.precisions]


class Config:      # config/config.py of the reference: what GPT reads of it is n_views (fuseattention.py:107)
    seq_len, n_views, vert_anchors, horz_anchors = 1, 1, 14, 14


def module(case, precision, pdrops=(0.0, 0.0, 0.0), use_pos=True, heads=None):
    """-> (fa.GPT on the GPU with the case's seeded parameters, its args, the parameter dict)"""
    from model import fuseattention as fa
    nv, v, h = ge.anchors(ge.tokens_of(case))

    class Cfg(Config):
        n_views, vert_anchors, horz_anchors = nv, v, h

    args = types.SimpleNamespace(arch="vit_small", pos_embed=use_pos)
    gpt = fa.GPT(case.dim, heads or case.heads, case.block_exp, case.depth, v, h, 1, *pdrops, args, Cfg(), precision=precision)
    assert gpt.n_tokens == ge.tokens_of(case)
    sd = ge.params_of(case)
    gpt.load_state_dict(sd, strict=True)
    return gpt.to(DEV), args, sd


def run(gpt, fc, fe, r):
    """one forward + backward of loss = sum(cat(a, b) * r) -> (a, b, {name: grad, "d.cxr", "d.enh"})"""
    for p in gpt.parameters():
        p.grad = None
    fc, fe = fc.to(DEV).requires_grad_(True), fe.to(DEV).requires_grad_(True)
    a, b = gpt(fc, fe)
    (torch.cat([a, b], 1) * r.to(DEV)).sum().backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in gpt.named_parameters()}
    grads["d.cxr"], grads["d.enh"] = fc.grad, fe.grad
    return a.detach(), b.detach(), grads


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name,precision", CASE_PRECISION, ids=[f"{n}-{p}" for n, p in CASE_PRECISION])
def test_parity_of_every_case(name, precision):
    """Forward, d tokens (both halves) and every parameter gradient of every case x precision through fa.GPT against the float64 oracle.
    Outputs in the max norm; gradients behind the ReLU MLP in l2 plus the capped share of entries past the entry-wise bound - caps the
    reference alone meets with half to spare at the operand type's accuracy (test_gpt_edges_cpu.py)."""
    case = ge.BY_NAME[name]
    tol, tol_g = ge.TOL[precision], ge.TOL_G[precision]
    gpt, args, _ = module(case, precision, use_pos=case.use_pos[0])
    gpt.train()                                            # all pdrop = 0: training mode is allowed
    fc, fe, r = ge.inputs_of(case)
    lines, checks = [], []
    engine = None
    for use_pos in case.use_pos:
        args.pos_embed = use_pos
        a, b, got = run(gpt, fc, fe, r)
        assert engine is None or gpt._engine is not engine             # a flipped args.pos_embed rebuilds the engine
        engine = gpt._engine
        assert a.shape == (case.B, case.split[0], case.dim) and b.shape == (case.B, case.split[1], case.dim)
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert all(g is None or bool(torch.isfinite(g).all()) for g in got.values())
        gp = got["pos_emb"]
        if use_pos:
            assert gp is not None and float(gp.abs().max()) > 0
        else:
            assert gp is None or not bool(gp.any())
        ref = ge.reference(name, use_pos)
        e_o = max(ge.scale_err(a, ref["a"]), ge.scale_err(b, ref["b"]))
        e = ge.grad_errors(got, ref["grads"], tol_g)
        lines.append(f"pos {'on' if use_pos else 'off'}: out {e_o:.2e} (< {tol:.1e}); {ge.fmt(e)} (L2 < {ge.L2_FACTOR * tol_g:.1e}, share <= {ge.OUTLIER_CAP:.0e})")
        checks.append((e_o, e))
    ge.log(f"GPT edges parity [{name}, {precision}] " + " | ".join(lines))
    for e_o, e in checks:
        assert e_o < tol, (e_o, tol)
        assert e.l2_tokens < ge.L2_FACTOR * tol_g and e.l2_param < ge.L2_FACTOR * tol_g, e
        assert e.out_tokens <= ge.OUTLIER_CAP and e.out_param <= ge.OUTLIER_CAP, e


# ------------------------------------------------------------------ (b)
@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
@pytest.mark.parametrize("name", ["tiny", "hd32", "wide"])
def test_dropout_at_the_edges(name, precision):
    """Training-mode dropout (0.1 at every site) at M = 5, at 12 heads x 32 - where attention dropout forces the streaming kernels and a
    plain-dtype qkv on a shape that otherwise runs whole-head with the split-fp16 qkv - and at width 768: the keep masks of THIS forward
    (mfvit_dropout_mask at sites 1, 16 l + 2, 16 l + 3, 16 l + 4) are handed to the float64 oracle.  Thresholds: those of
    test_transfuser_gpu.py::test_gpt_training_mode_dropout_matches_reference_with_the_same_masks."""
    from mfvit import ops
    case = ge.BY_NAME[name]
    tol = {"bf16x3": 2e-3, "fp16": 2e-2}[precision]
    pdrops = (0.1, 0.1, 0.1)
    B, T, C, H = case.B, ge.tokens_of(case), case.dim, case.heads
    gpt, _, sd = module(case, precision, pdrops)
    gpt.train()
    fc, fe, r = ge.inputs_of(case)
    torch.manual_seed(case.seed)                           # the module draws its mask seed from torch's generator: the same masks on every run
    a, b, got = run(gpt, fc, fe, r)
    seed = gpt._last_drop[3]
    drop = {"embd": ops.dropout_mask(pdrops[0], seed, 1, B * T * C).reshape(B, T, C).cpu()}
    for l in range(case.depth):
        drop[("attn", l)] = ops.dropout_mask(pdrops[1], seed, 16 * l + 2, B * H * T * T).reshape(B, H, T, T).cpu()
        drop[("proj", l)] = ops.dropout_mask(pdrops[2], seed, 16 * l + 3, B * T * C).reshape(B, T, C).cpu()
        drop[("mlp", l)] = ops.dropout_mask(pdrops[2], seed, 16 * l + 4, B * T * C).reshape(B, T, C).cpu()
    if name != "tiny":                                     # (tiny: the attention site has 1 * 4 * 5 * 5 = 100 mask elements)
        for k, m in drop.items():
            rate = m.double().mean().item()
            assert abs(rate - 0.9) < 4 * (0.1 * 0.9 / m.numel()) ** 0.5 + 1e-4, (k, rate)
    ref = ge.run_reference(case, sd, fc, fe, r, drop=drop, pdrops=pdrops)
    e_o = max(ge.scale_err(a, ref["a"]), ge.scale_err(b, ref["b"]))
    e = ge.grad_errors(got, ref["grads"], tol)
    ge.log(f"GPT edges dropout [{name}, {precision}, p={pdrops}]: out {e_o:.2e} (< {tol:.1e}); {ge.fmt(e)} (L2 < {5 * tol:.1e}, share < 5e-02)")
    assert e_o < tol and e.l2_tokens < 5 * tol and e.l2_param < 5 * tol and e.out_tokens < 5e-2 and e.out_param < 5e-2, (e_o, e)
    # the masks matter: the dropout-free reference is far away
    assert ge.scale_err(a, ge.reference(name)["a"]) > 10 * tol
    if name == "hd32":
        # the same module, the same engine, in eval(): the whole-head kernels behind the split-fp16 qkv epilogue, against the mask-free oracle
        engine = gpt._engine
        gpt.eval()
        a, b, got = run(gpt, fc, fe, r)
        assert gpt._engine is engine
        ref = ge.reference(name)
        e_o = max(ge.scale_err(a, ref["a"]), ge.scale_err(b, ref["b"]))
        e = ge.grad_errors(got, ref["grads"], ge.TOL_G[precision])
        ge.log(f"GPT edges dropout [{name}, {precision}] the same engine in eval(): out {e_o:.2e} (< {ge.TOL[precision]:.1e}); {ge.fmt(e)}")
        assert e_o < ge.TOL[precision], e_o
        assert max(e.l2_tokens, e.l2_param) < ge.L2_FACTOR * ge.TOL_G[precision] and max(e.out_tokens, e.out_param) <= ge.OUTLIER_CAP, e


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("precision", ge.BY_NAME["blk129"].precisions)
def test_samples_are_independent_and_gradients_add(precision):
    """blk129 at B = 3 (M = 387): every sample of the batch comes out as it does alone (bounds and additivity tolerances of
    test_encoder_gpu.py::test_full_size_batch_is_sample_independent: the row kernels switch form with the row count, so an f32 last-bit
    difference may flip a rounding of the operand type), grad(B = 3) = grad(samples 0 - 1) + grad(sample 2), and a repeated run returns
    the same bits."""
    case = ge.BY_NAME["blk129"]
    gpt, _, _ = module(case, precision)
    gpt.train()
    fc, fe, r = ge.inputs_of(case, B=3)
    fwd_tol = {"bf16x3": 1e-4, "bf16": 1e-2, "fp16": 2e-3}
    add_tol = {"bf16": 2e-2, "fp16": 5e-3, "bf16x3": 1e-3, "fp32": 1e-4}[precision]
    with torch.no_grad():
        full = torch.cat(gpt(fc.to(DEV), fe.to(DEV)), 1)
        worst_f = 0.0
        for s in (0, 2):
            part = torch.cat(gpt(fc[s:s + 1].to(DEV), fe[s:s + 1].to(DEV)), 1)
            if precision == "fp32":
                assert torch.equal(full[s:s + 1], part), s
            else:
                e = ((full[s:s + 1] - part).abs().max() / part.abs().max()).item()
                worst_f = max(worst_f, e)
                assert e < fwd_tol[precision], (s, e)
    assert torch.isfinite(full).all()
    a3, b3, g3 = run(gpt, fc, fe, r)
    _, _, g01 = run(gpt, fc[:2], fe[:2], r[:2])
    _, _, g2 = run(gpt, fc[2:], fe[2:], r[2:])
    # error over the tensor's largest entry - or, for a gradient that is mathematically zero (attn.key.bias: rounding noise in every run), over
    # the floor of the error measures, 1e-3 of the largest parameter gradient
    floor = 1e-3 * max(float(v.abs().max()) for k, v in g3.items() if not k.startswith("d."))
    worst = ("", 0.0)
    for k in g3:
        want = torch.cat([g01[k], g2[k]], 0) if k.startswith("d.") else g01[k] + g2[k]
        e = float((g3[k] - want).abs().max()) / max(float(want.abs().max()), floor)
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < add_tol, (k, e)
    a3b, b3b, g3b = run(gpt, fc, fe, r)
    assert torch.equal(a3, a3b) and torch.equal(b3, b3b)
    for k in g3:
        assert torch.equal(g3[k], g3b[k]), k
    ge.log(f"GPT edges sample independence [blk129 at B = 3, {precision}]: forward {worst_f:.2e} (< {fwd_tol.get(precision, 0):.0e}), "
           f"gradient additivity worst {worst[0]} {worst[1]:.2e} (< {add_tol:.0e}), repeated run bit-identical")


# ------------------------------------------------------------------ (d) the C ABI directly
class Abi:
    """One cfg's buffers and calls on mfvit._lib, the way mfvit/gpt.py::GptEngine makes them."""

    def __init__(self, case, precision, act=1, use_pos=1, save=1):
        from mfvit import _lib
        self.L, self.lib = _lib, _lib.lib()
        self.case, self.cfg = case, ge.make_cfg(case, precision, save=save, use_pos=use_pos, act=act)
        self.flat, self.where = ge.flat_arena(case, ge.params_of(case))
        self.flat = self.flat.to(DEV)
        assert self.lib.mfvit_vit_param_count(self.cfg) == self.flat.numel()
        self.shadow = torch.empty(self.lib.mfvit_vit_shadow_bytes(self.cfg), device=DEV, dtype=torch.uint8)
        _lib.check(self.lib.mfvit_vit_prepare_shadow(self.cfg, _lib.ptr(self.flat), _lib.ptr(self.shadow), _lib.stream()), "mfvit_vit_prepare_shadow")
        self.ws = torch.empty(self.lib.mfvit_vit_workspace_bytes(self.cfg), device=DEV, dtype=torch.uint8)
        fc, fe, r = ge.inputs_of(case)
        self.tokens, self.dout = torch.cat([fc, fe], 1).contiguous().to(DEV), r.contiguous().to(DEV)

    def forward(self, cfg=None):
        p = self.L.ptr
        out = torch.full_like(self.tokens, float("nan"))
        rc = self.lib.mfvit_gpt_forward(cfg or self.cfg, p(self.flat), p(self.shadow), p(self.tokens), p(self.ws), p(out), self.L.stream())
        return rc, out

    def backward(self, dparams, cfg=None, dout="own", dtokens="own"):
        p = self.L.ptr
        dt = torch.full_like(self.tokens, float("nan")) if isinstance(dtokens, str) else dtokens
        do = self.dout if isinstance(dout, str) else dout
        rc = self.lib.mfvit_gpt_backward(cfg or self.cfg, p(self.flat), p(self.shadow), p(self.ws), p(do), p(dparams), p(dt), self.L.stream())
        return rc, dt

    def grads_of(self, dparams, dtokens):
        n0 = self.case.split[0]
        g = {k: dparams[off:off + int(torch.Size(shape).numel())].view(shape) for k, (off, shape) in self.where.items()}
        g["d.cxr"], g["d.enh"] = dtokens[:, :n0], dtokens[:, n0:]
        return g


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_abi_gelu_variant_in_the_max_norm_and_accumulated_dparams(precision):
    """act = 0 (erf-GELU), reachable through the C ABI only: nothing on the way is discontinuous, so the forward and EVERY gradient are held
    to max-norm bounds with no outlier allowance.  out / dtokens start as NaN: every entry is written.  dparams is ACCUMULATED: on an arena
    pre-filled with g0 the result is g0 + grad, grad from a second call on a zeroed arena, to f32 rounding (1e-6 max|.| per tensor)."""
    case = ge.BY_NAME["hd64"]
    tol, tol_g = ge.TOL[precision], ge.TOL_G[precision]
    x = Abi(case, precision, act=0)
    rc, out = x.forward()
    assert rc == 0 and torch.isfinite(out).all()
    grad = torch.zeros_like(x.flat)
    rc, dtok = x.backward(grad)
    assert rc == 0 and torch.isfinite(dtok).all() and torch.isfinite(grad).all()
    ref = ge.reference("hd64", True, "gelu")
    n0 = case.split[0]
    e_o = max(ge.scale_err(out[:, :n0], ref["a"]), ge.scale_err(out[:, n0:], ref["b"]))
    got = x.grads_of(grad, dtok)
    e = ge.grad_errors(got, ref["grads"], tol_g)
    ge.log(f"GPT edges C ABI [hd64, {precision}, act 0 = erf-GELU]: out {e_o:.2e} (< {tol:.1e}); gradients, max norm: worst {e.max_name} {e.max_all:.2e} "
           f"(< {tol_g:.1e}); entries past tolerance {max(e.out_tokens, e.out_param):.1e}")
    assert e_o < tol, e_o
    assert e.max_all < tol_g, e
    # not the ReLU network: the same call with act = 1 is far from this reference
    y = Abi(case, precision, act=1)
    rc, out_relu = y.forward()
    assert rc == 0 and ge.scale_err(out_relu[:, :n0], ref["a"]) > 10 * tol
    # accumulate: g0 at every tensor's own gradient scale (the floor keeps the mathematically-zero ones non-trivial)
    gmax = float(grad.abs().max())
    g0 = rng_tensor(case.seed + 50, (x.flat.numel(),)).to(DEV)
    for k, (off, shape) in x.where.items():
        n = int(torch.Size(shape).numel())
        g0[off:off + n] *= max(float(grad[off:off + n].abs().max()), 1e-3 * gmax)
    acc = g0.clone()
    rc, _ = x.forward()
    assert rc == 0
    rc, dtok2 = x.backward(acc)
    assert rc == 0 and torch.equal(dtok2, dtok)
    worst = ("", 0.0)
    for k, (off, shape) in x.where.items():
        n = int(torch.Size(shape).numel())
        want = g0[off:off + n].double() + grad[off:off + n].double()
        err = float((acc[off:off + n].double() - want).abs().max() / want.abs().max().clamp_min(1e-30))
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert err < 1e-6, (k, err)
        assert float((acc[off:off + n] - g0[off:off + n]).abs().max()) > 0 or float(grad[off:off + n].abs().max()) == 0, k
    ge.log(f"GPT edges C ABI [hd64, {precision}] dparams accumulated: worst {worst[0]} {worst[1]:.2e} of max|g0 + grad| (< 1e-6)")


@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
def test_abi_writes_every_row_at_five_rows(precision):
    """M = 5: below every GEMM tile, row-kernel tile and weight-gradient stage - every entry of out and dtokens is written, and agrees."""
    case = ge.BY_NAME["tiny"]
    x = Abi(case, precision)
    rc, out = x.forward()
    assert rc == 0 and torch.isfinite(out).all()
    grad = torch.zeros_like(x.flat)
    rc, dtok = x.backward(grad)
    assert rc == 0 and torch.isfinite(dtok).all() and torch.isfinite(grad).all()
    ref = ge.reference("tiny")
    n0 = case.split[0]
    assert max(ge.scale_err(out[:, :n0], ref["a"]), ge.scale_err(out[:, n0:], ref["b"])) < ge.TOL[precision]
    e = ge.grad_errors(x.grads_of(grad, dtok), ref["grads"], ge.TOL_G[precision])
    assert max(e.l2_tokens, e.l2_param) < ge.L2_FACTOR * ge.TOL_G[precision], e


def test_abi_argument_errors_launch_nothing():
    case = ge.BY_NAME["hd64"]
    x = Abi(case, "bf16x3")
    rc, out = x.forward()
    assert rc == 0
    L, lib, p = x.L, x.lib, x.L.ptr
    g0 = rng_tensor(case.seed + 60, (x.flat.numel(),)).to(DEV)
    dparams = g0.clone()
    nan = torch.full_like(x.tokens, float("nan"))
    assert x.backward(dparams, dout=None)[0] == EINVAL
    assert x.backward(None)[0] == EINVAL
    assert x.backward(dparams, dtokens=None)[0] == EINVAL
    nosave = ge.make_cfg(case, "bf16x3", save=0)
    rc, dt = x.backward(dparams, cfg=nosave)
    assert rc == EINVAL and torch.isnan(dt).all()
    # the image encoder's backward on a token cfg, the GPT's entry points on an image cfg
    assert lib.mfvit_vit_backward(x.cfg, p(x.flat), p(x.shadow), p(x.ws), p(x.dout), p(dparams), case.depth, -1, L.stream()) == EINVAL
    img = L.VitCfg()
    img.dtype, img.batch, img.img_h, img.img_w, img.dim, img.depth, img.heads, img.mlp_dim = L.BF16X3, 1, 32, 32, 384, 2, 6, 1536
    img.save_for_backward, img.ln_eps = 1, 1e-6
    assert lib.mfvit_vit_workspace_bytes(img) > 0
    rc, dt = x.backward(dparams, cfg=img)
    assert rc == EINVAL and torch.isnan(dt).all()
    rc, o = x.forward(cfg=img)
    assert rc == EINVAL and torch.isnan(o).all()
    assert lib.mfvit_vit_forward(x.cfg, p(x.flat), p(x.shadow), p(x.tokens), p(x.ws), p(nan), L.stream()) == EINVAL and torch.isnan(nan).all()
    # fp32 past the exact attention's LDS image (6 heads x 64 at the model's own 394 tokens; T <= 315): refused before the first launch
    long = ge.make_cfg(case, "fp32", tokens=394)
    assert lib.mfvit_vit_workspace_bytes(long) == 0
    rc, o = x.forward(cfg=long)
    assert rc == EINVAL and torch.isnan(o).all()
    rc, dt = x.backward(dparams, cfg=long)
    assert rc == EINVAL and torch.isnan(dt).all()
    torch.cuda.synchronize()
    assert torch.equal(dparams, g0)                         # none of the refused calls touched the gradient arena
    # ... and the module says so in its own words
    big = ge.BY_NAME["model_bf16"]
    gpt, _, _ = module(big, "fp32", heads=6)
    fc, fe, _ = ge.inputs_of(big)
    with pytest.raises(L.MfvitError, match="invalid GPT configuration"):
        gpt(fc.to(DEV), fe.to(DEV))
