"""CPU side of the token-input (GPT) encoder's edge suite (tests/gpt_edges_ref.py holds the case table; tests/test_gpt_edges_gpu.py the parity):
  (a) the gradient caps of the GPU parity are met by the float64 reference ALONE when its weights carry the operand type's product noise -
      what makes "at most 5 % of a tensor's entries past the bound" a condition on the kernels and not a loophole;
  (b) the host-only queries of the C ABI for every case, and the refusals outside the domain;
  (c) the fp32 sequence limit: the exact attention's LDS image, refused by the size queries, not inside block 0."""
import ctypes
import types

import pytest
import torch

import gpt_edges_ref as ge
from conftest import rng_tensor
from oracle import ref_gpt

EINVAL = -22
CASE_PRECISION = [(c.name, p) for c in ge.CASES for p in c.precisions]


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name,precision", CASE_PRECISION, ids=[f"{n}-{p}" for n, p in CASE_PRECISION])
def test_reference_alone_meets_half_of_every_cap(name, precision):
    """float64 oracle against ITSELF with every weight matrix multiplied by 1 + eps N(0, 1), eps = one product of the operand type: the ReLU
    units that switch side at that accuracy.  Must stay below HALF of each gradient threshold of the GPU parity (l2 < 2.5 tol_g, at most 2.5 %
    of a tensor's entries past 2 tol_g max|ref|) - a seed or shape that does not is changed in the table, never the threshold."""
    case = ge.BY_NAME[name]
    eps, tol_g = ge.PRODUCT_NOISE[precision], ge.TOL_G[precision]
    base = ge.params_of(case)
    noisy = {}
    for i, (k, v) in enumerate(base.items()):
        noisy[k] = v * (1.0 + eps * rng_tensor(case.seed + 100 + i, tuple(v.shape), dtype=torch.float64)) if v.dim() == 2 else v
    for use_pos in case.use_pos:
        ref = ge.reference(name, use_pos)
        got = ge.run_reference(case, noisy, *ge.inputs_of(case), use_pos=use_pos)
        e = ge.grad_errors(got["grads"], ref["grads"], tol_g)
        e_o = max(ge.scale_err(got["a"], ref["a"]), ge.scale_err(got["b"], ref["b"]))
        print(f"reference vs itself [{name}, {precision}, pos {use_pos}, eps {eps:.1e}]: out {e_o:.2e}; {ge.fmt(e)}")
        assert max(e.l2_tokens, e.l2_param) < 0.5 * ge.L2_FACTOR * tol_g, e
        assert max(e.out_tokens, e.out_param) < 0.5 * ge.OUTLIER_CAP, e


def test_selectable_activation_leaves_the_relu_reference_as_it_was():
    case = ge.BY_NAME["tiny"]
    p = {k: v.double() for k, v in ge.params_of(case).items()}
    fc, fe, _ = ge.inputs_of(case)
    a0, b0 = ref_gpt.gpt_forward(p, fc.double(), fe.double(), n_head=case.heads)
    a1, b1 = ref_gpt.gpt_forward(p, fc.double(), fe.double(), n_head=case.heads, act="relu")
    a2, _ = ref_gpt.gpt_forward(p, fc.double(), fe.double(), n_head=case.heads, act="gelu")
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and not torch.equal(a0, a2)
    assert a0.shape == (1, 2, 384) and b0.shape == (1, 3, 384)


# ------------------------------------------------------------------ (b)
def _L():
    from mfvit import _lib
    return _lib


def _layout(cfg):
    out = (ctypes.c_int64 * 9)()
    return _L().lib().mfvit_vit_param_layout(cfg, out), list(out)


def _refused(cfg):
    lib = _L().lib()
    rc, _ = _layout(cfg)
    return (lib.mfvit_vit_workspace_bytes(cfg), lib.mfvit_vit_shadow_bytes(cfg), lib.mfvit_vit_param_count(cfg), rc) == (0, 0, 0, EINVAL)


def _accepted(cfg):
    lib = _L().lib()
    rc, _ = _layout(cfg)
    return lib.mfvit_vit_workspace_bytes(cfg) > 0 and lib.mfvit_vit_shadow_bytes(cfg) > 0 and lib.mfvit_vit_param_count(cfg) > 0 and rc == 0


@pytest.mark.parametrize("name,precision", CASE_PRECISION, ids=[f"{n}-{p}" for n, p in CASE_PRECISION])
def test_host_queries_of_every_case(name, precision):
    case = ge.BY_NAME[name]
    lib = _L().lib()
    T = ge.tokens_of(case)
    shapes = ref_gpt.gpt_param_shapes(n_embd=case.dim, block_exp=case.block_exp, n_layer=case.depth, n_tokens=T)
    assert sorted(shapes) == sorted(ge.arena_names(case))
    total = sum(int(torch.Size(s).numel()) for s in shapes.values())
    per_block = (total - T * case.dim - 2 * case.dim) // case.depth
    for use_pos in (0, 1):
        cfg = ge.make_cfg(case, precision, use_pos=use_pos)
        assert lib.mfvit_vit_param_count(cfg) == total
        rc, L = _layout(cfg)
        # [0] cls (none) = [1] pos_emb = 0; [2] = [3] (no patch embedding) = [4] the first block, behind pos_emb; [5] block stride; [6] [7] ln_f; [8] total
        assert rc == 0 and L[0] == L[1] == 0 and L[2] == L[3] == L[4] == T * case.dim, L
        assert L[5] == per_block and L[6] == L[4] + case.depth * per_block and L[7] == L[6] + case.dim and L[8] == total, L
        assert lib.mfvit_vit_workspace_bytes(cfg) > 0 and lib.mfvit_vit_shadow_bytes(cfg) > 0
        assert lib.mfvit_vit_workspace_bytes(ge.make_cfg(case, precision, use_pos=use_pos, save=0)) > 0
    # the flat arena of the helpers is that layout
    flat, where = ge.flat_arena(case, ge.params_of(case))
    assert flat.numel() == total and where["pos_emb"][0] == 0 and where["blocks.0.ln1.weight"][0] == T * case.dim
    assert where["ln_f.weight"][0] == L[6] and where["ln_f.bias"][0] == L[7]
    if case.depth > 1:
        assert where["blocks.1.ln1.weight"][0] - where["blocks.0.ln1.weight"][0] == per_block


def test_arena_order_is_the_modules():
    from model import fuseattention as fa
    case = ge.BY_NAME["hd64"]
    gpt = _module(fa, case, "bf16x3")
    assert [n for n, _ in gpt.arena_named_parameters()] == ge.arena_names(case)
    assert gpt.n_tokens == ge.tokens_of(case)
    for c in ge.CASES:
        nv, v, h = ge.anchors(ge.tokens_of(c))
        assert (nv + 1) * v * h + 2 == ge.tokens_of(c)


def _module(fa, case, precision):
    nv, v, h = ge.anchors(ge.tokens_of(case))
    config = types.SimpleNamespace(n_views=nv, seq_len=1, vert_anchors=v, horz_anchors=h)
    args = types.SimpleNamespace(arch="vit_small", pos_embed=True)
    return fa.GPT(case.dim, case.heads, case.block_exp, case.depth, v, h, 1, 0.0, 0.0, 0.0, args, config, precision=precision)


def test_attention_qkv_dtype_of_the_cases():
    L = _L()
    lib = L.lib()
    assert lib.mfvit_attention_qkv_dtype(L.BF16X3, 65, 32) == L.X3F16          # hd32: whole-head kernels, split-fp16 qkv
    for dt in (L.F32, L.BF16, L.F16):
        assert lib.mfvit_attention_qkv_dtype(dt, 65, 32) == dt
    for dt in (L.F32, L.BF16, L.BF16X3, L.F16):
        for T, hd in ((5, 96), (34, 64), (129, 96), (34, 96), (394, 96), (65, 64)):
            assert lib.mfvit_attention_qkv_dtype(dt, T, hd) == dt, (dt, T, hd)


def test_out_of_domain_is_refused_by_every_query():
    case = ge.BY_NAME["hd64"]
    assert _accepted(ge.make_cfg(case, "bf16x3")) and _accepted(ge.make_cfg(case, "fp32"))

    def variant(precision="bf16x3", **kw):
        c = ge.make_cfg(case, precision)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    bad = {"tokens 0": variant(tokens=0), "dim 512": variant(dim=512, heads=8, mlp_dim=2048), "head_dim 48": variant(heads=8),
           "mlp_dim 200": variant(mlp_dim=200), "fp32 head_dim 96": variant("fp32", heads=4), "fp32 with dropout": variant("fp32", p_resid=0.1),
           "rate 1.0": variant(p_attn=1.0), "act 2": variant(act=2)}
    for what, cfg in bad.items():
        assert _refused(cfg), what
    # the same changes one step inside the domain are accepted
    for what, cfg in {"tokens 1": variant(tokens=1), "dim 768": variant(dim=768, heads=12, mlp_dim=256), "head_dim 32": variant(heads=12),
                      "mlp_dim 128": variant(mlp_dim=128), "bf16x3 head_dim 96": variant(heads=4), "bf16 with dropout": variant("bf16", p_resid=0.1),
                      "rate 0.99": variant(p_attn=0.99), "act 0": variant(act=0)}.items():
        assert _accepted(cfg), what


def test_fp32_head_dim_96_still_raises_in_the_module():
    from model import fuseattention as fa
    with pytest.raises(NotImplementedError):
        _module(fa, ge.BY_NAME["tiny"], "fp32")._eng()
    _module(fa, ge.BY_NAME["tiny"], "bf16x3")                                  # (the same module in a 16-bit type builds)


# ------------------------------------------------------------------ (c)
def _image_cfg(precision, heads, h, w, dim=384):
    c = _L().VitCfg()
    c.dtype = _L().dtype_code(precision)
    c.batch, c.img_h, c.img_w = 1, h, w
    c.dim, c.depth, c.heads, c.mlp_dim = dim, 2, heads, 4 * dim
    c.save_for_backward, c.ln_eps = 1, 1e-6
    return c


# The exact attention of MFVIT_F32 (csrc/attention.hip) keeps K and V of one head in LDS: launch_fwd needs 2 T hd 4 bytes, launch_bwd
# 2 T hd 4 + 2 T 4 (two [T] vectors more), each at most 160 * 1024.  The backward's is the binding one - and the code's arithmetic is the
# issue's: hd 64: 520 T <= 163,840 -> T <= 315; hd 32: 264 T <= 163,840 -> T <= 620.
@pytest.mark.parametrize("heads,t_ok", [(6, 315), (12, 620)])
def test_fp32_sequence_limit_token_mode(heads, t_ok):
    hd = 384 // heads
    assert 2 * t_ok * hd * 4 + 8 * t_ok <= 160 * 1024 < 2 * (t_ok + 1) * hd * 4 + 8 * (t_ok + 1)
    case = ge.BY_NAME["hd64"]._replace(heads=heads)
    assert _accepted(ge.make_cfg(case, "fp32", tokens=t_ok))
    assert _refused(ge.make_cfg(case, "fp32", tokens=t_ok + 1))
    assert _refused(ge.make_cfg(case, "fp32", tokens=394 if heads == 6 else 1000))
    for precision in ("bf16x3", "fp16", "bf16"):                               # the streaming kernels take any length
        assert _accepted(ge.make_cfg(case, precision, tokens=t_ok + 1)) and _accepted(ge.make_cfg(case, precision, tokens=4096))


@pytest.mark.parametrize("heads,ok_hw,bad_hw", [(6, (32, 2512), (240, 336)), (12, (16, 9904), (320, 496))])
def test_fp32_sequence_limit_image_mode(heads, ok_hw, bad_hw):
    """T = 1 + patches: 315 / 316 at head_dim 64, 620 / 621 at head_dim 32 - and 400 x 400 inputs (T = 626) in fp32 with 12 heads."""
    t_ok = 315 if heads == 6 else 620
    assert (ok_hw[0] // 16) * (ok_hw[1] // 16) + 1 == t_ok and (bad_hw[0] // 16) * (bad_hw[1] // 16) + 1 == t_ok + 1
    assert _accepted(_image_cfg("fp32", heads, *ok_hw))
    assert _refused(_image_cfg("fp32", heads, *bad_hw))
    assert _refused(_image_cfg("fp32", heads, 400, 400))
    assert _accepted(_image_cfg("fp32", heads, 224, 224))
    for precision in ("bf16x3", "fp16", "bf16"):
        assert _accepted(_image_cfg(precision, heads, *bad_hw)) and _accepted(_image_cfg(precision, heads, 400, 400))
    lib = _L().lib()
    drop = _L().VitDrop()
    assert lib.mfvit_vit_workspace_bytes_drop(_image_cfg("fp32", heads, *bad_hw), drop) == 0
    assert lib.mfvit_vit_workspace_bytes_ex(_image_cfg("fp32", heads, *bad_hw), None, 1) == 0
    assert lib.mfvit_vit_workspace_bytes_ex(_image_cfg("fp32", heads, *ok_hw), None, 1) > 0
