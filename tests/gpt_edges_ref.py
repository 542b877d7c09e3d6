"""The case table and the reference helpers of tests/test_gpt_edges_gpu.py and tests/test_gpt_edges_cpu.py: the token-input (GPT) encoder
(model/fuseattention.py -> mfvit/gpt.py -> mfvit_gpt_forward / mfvit_gpt_backward) at its token, head and width edges.  Not a test module.

The reference is oracle/ref_gpt.py::gpt_forward in float64 with autograd; parameters are ref_gpt.seeded_gpt_params, tokens and the upstream
gradient conftest.rng_tensor.  One reference per (case, pos_emb on / off, activation) is computed per process and shared by every test that
needs it (lru_cache): nobody writes to it.

Error measures (those of test_transfuser_gpu.py::test_gpt_training_mode_dropout_matches_reference_with_the_same_masks):
  scale_err   max |got - ref| / max |ref|                                   outputs (and, for the GELU variant, gradients)
  l2          |got - ref|_2 / |ref|_2 per tensor                            gradients behind the ReLU MLP
  outliers    share of a tensor's entries with |got - ref| > 2 tol_g max|ref|
Tensors whose reference gradient is below 1e-3 of the largest parameter gradient are skipped, as there: attn.key.bias is mathematically
zero (a shift of every key leaves the softmax unchanged) and is rounding noise on both sides.
"""
import collections
import functools
import os

import torch

from conftest import rng_tensor
from oracle import ref_gpt

# per precision: outputs (test_transfuser_gpu.py, test_unfused_gpu.py, test_encoder_gpu.py) and gradients
TOL = {"bf16x3": 1e-3, "fp16": 1.5e-2, "bf16": 4e-2, "fp32": 1e-3}
TOL_G = {"bf16x3": 2e-3, "fp16": 2e-2, "bf16": 8e-2, "fp32": 2e-3}
L2_FACTOR = 5.0          # gradients: l2 < 5 tol_g ...
OUTLIER_CAP = 5e-2       # ... and at most 5 % of a tensor's entries past the entry-wise bound
# The accuracy of one product of the operand type = the relative noise put on every weight matrix when the float64 reference is compared
# with ITSELF (test_gpt_edges_cpu.py): what a ReLU unit switching side costs at that accuracy, with no kernel involved.  bf16x3: the 1e-5
# test_transfuser_gpu.py documents (hi + lo = 16 mantissa bits); fp16 2^-11; bf16 2^-8; fp32 2^-24.
PRODUCT_NOISE = {"bf16x3": 1e-5, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp32": 2.0 ** -24}

ALL4 = ("bf16x3", "fp16", "bf16", "fp32")
Case = collections.namedtuple("Case", "name B split dim heads block_exp depth use_pos precisions seed")
# use_pos: the args.pos_embed settings one module runs through, in order (a flip rebuilds the engine).  seed: of the parameters; the
# tokens and the upstream gradient take seed + 1 .. seed + 3.  Depth 2: block 0's `l == 0` branches and a block with a predecessor.
# Rejected seeds (test_gpt_edges_cpu.py::test_reference_alone_meets_half_of_every_cap): tiny 1100 - at fp16 noise one ReLU unit of its 5 rows
# switches side and 12 of the 384 entries of blocks.0.attn.query.bias (3.1 %, half the cap is 2.5 %) pass the bound; 1101, the next, is taken.
CASES = (
    # M = 5: below every tile, chunk and stage; one partial 32-row attention tile
    Case("tiny", 1, (2, 3), 384, 4, 3, 2, (True,), ("bf16x3", "fp16", "bf16"), 1101),
    # the 64x64-image token count; pos_emb row-modulo at B = 3; fp32: the exact attention
    Case("hd64", 3, (17, 17), 384, 6, 4, 2, (False, True), ALL4, 1200),
    # whole-head MFMA kernels; X3F16 qkv epilogue in bf16x3; M = 130: two rows into a second 128-row tile; mlp_dim 384; T one past a 64-row chunk
    Case("hd32", 2, (33, 32), 384, 12, 1, 2, (True,), ALL4, 1300),
    # one row into the second 128-row block of the streaming kernels
    Case("blk129", 2, (65, 64), 384, 4, 3, 2, (True,), ("bf16x3", "fp16", "bf16"), 1400),
    # unfused rows + ReLU at width 768
    Case("wide", 2, (17, 17), 768, 8, 2, 2, (True,), ("bf16x3", "fp16"), 1500),
    # the same with the exact / streaming head_dim-64 attention
    Case("wide64", 2, (17, 17), 768, 12, 2, 2, (True,), ("fp32", "bf16"), 1600),
    # the model's own shape in the one 16-bit type never run through the composite
    Case("model_bf16", 1, (197, 197), 384, 4, 3, 1, (True,), ("bf16",), 1700),
)
BY_NAME = {c.name: c for c in CASES}


def tokens_of(case):
    return case.split[0] + case.split[1]


def anchors(T):
    """(n_views, vert_anchors, horz_anchors) with (n_views + 1) * vert * horz + 2 == T at seq_len 1 (fuseattention.py:107)."""
    known = {5: (2, 1, 1), 34: (1, 4, 4), 394: (1, 14, 14)}
    nv, v, h = known.get(T, (T - 3, 1, 1))
    assert nv >= 0 and (nv + 1) * v * h + 2 == T, T
    return nv, v, h


def make_cfg(case, precision, B=None, save=1, use_pos=1, act=1, tokens=None):
    """The mfvit_vit_cfg of a case in token-input mode, as mfvit/gpt.py::GptEngine.cfg fills it (act: 1 ReLU, 0 erf-GELU)."""
    from mfvit import _lib
    c = _lib.VitCfg()
    c.dtype = _lib.dtype_code(precision)
    c.batch, c.img_h, c.img_w = B or case.B, 0, 0
    c.dim, c.depth, c.heads, c.mlp_dim = case.dim, case.depth, case.heads, case.block_exp * case.dim
    c.save_for_backward, c.stop_grad_conv1, c.ln_eps = save, 0, 1e-5
    c.token_input, c.tokens, c.use_pos, c.act = 1, tokens or tokens_of(case), use_pos, act
    return c


def arena_names(case):
    """Parameter names in the C ABI's arena order (include/mfvit.h, mfvit_gpt_forward; model/fuseattention.py::GPT.arena_named_parameters)."""
    out = ["pos_emb"]
    for i in range(case.depth):
        p = f"blocks.{i}."
        out += [p + "ln1.weight", p + "ln1.bias", p + "attn.query.weight", p + "attn.key.weight", p + "attn.value.weight", p + "attn.query.bias",
                p + "attn.key.bias", p + "attn.value.bias", p + "attn.proj.weight", p + "attn.proj.bias", p + "ln2.weight", p + "ln2.bias",
                p + "mlp.0.weight", p + "mlp.0.bias", p + "mlp.2.weight", p + "mlp.2.bias"]
    return out + ["ln_f.weight", "ln_f.bias"]


def flat_arena(case, params):
    """The f32 arena of a parameter dict and {name: (offset, shape)}."""
    off, where, parts = 0, {}, []
    for k in arena_names(case):
        where[k] = (off, tuple(params[k].shape))
        parts.append(params[k].reshape(-1).float())
        off += params[k].numel()
    return torch.cat(parts), where


def params_of(case):
    return ref_gpt.seeded_gpt_params(case.seed, n_embd=case.dim, block_exp=case.block_exp, n_layer=case.depth, n_tokens=tokens_of(case))


def inputs_of(case, B=None):
    """(cxr tokens, enh tokens, upstream gradient) in f32 on the CPU; B overrides the case's batch (sample-independence test)."""
    B = B or case.B
    fc = rng_tensor(case.seed + 1, (B, case.split[0], case.dim))
    fe = rng_tensor(case.seed + 2, (B, case.split[1], case.dim))
    r = rng_tensor(case.seed + 3, (B, tokens_of(case), case.dim))
    return fc, fe, r


def run_reference(case, params, fc, fe, r, use_pos=True, act="relu", drop=None, pdrops=(0.0, 0.0, 0.0), n_head=None):
    """float64 forward + backward of loss = sum(cat(a, b) * r).  -> {"a", "b", "grads": {name: grad, "d.cxr", "d.enh"}}; a parameter
    that takes no part (pos_emb with use_pos off) has no entry."""
    pd = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    fcd, fed = fc.detach().double().cpu().clone().requires_grad_(True), fe.detach().double().cpu().clone().requires_grad_(True)
    a, b = ref_gpt.gpt_forward(pd, fcd, fed, n_head=n_head or case.heads, pos_embed=use_pos, drop=drop, pdrops=pdrops, act=act)
    (torch.cat([a, b], 1) * r.detach().double().cpu()).sum().backward()
    grads = {k: v.grad for k, v in pd.items() if v.grad is not None}
    grads["d.cxr"], grads["d.enh"] = fcd.grad, fed.grad
    return {"a": a.detach(), "b": b.detach(), "grads": grads}


@functools.lru_cache(maxsize=None)
def reference(name, use_pos=True, act="relu"):
    """The dropout-free reference of a case at its own batch: computed once per process, read-only."""
    case = BY_NAME[name]
    return run_reference(case, params_of(case), *inputs_of(case), use_pos=use_pos, act=act)


def scale_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def outliers(got, ref, tol_g):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() > 2 * tol_g * float(ref.abs().max())).double().mean())


def grad_floor(ref_grads):
    """1e-3 of the largest PARAMETER gradient: reference gradients below it are rounding noise on both sides."""
    return 1e-3 * max(float(v.abs().max()) for k, v in ref_grads.items() if not k.startswith("d."))


GradErr = collections.namedtuple("GradErr", "l2_tokens out_tokens l2_param l2_name out_param out_name max_all max_name")


def grad_errors(got, ref_grads, tol_g):
    """got: {name: tensor} with every key of ref_grads.  -> GradErr: the worst l2 / outlier share of d tokens and of the parameters, and the
    worst scale_err of all (the GELU variant's measure)."""
    floor = grad_floor(ref_grads)
    w = {"l2t": 0.0, "ot": 0.0, "l2p": (0.0, ""), "op": (0.0, ""), "mx": (0.0, "")}
    for k, ref in ref_grads.items():
        if float(ref.abs().max()) < floor:
            continue
        assert got[k] is not None and got[k].shape == ref.shape, k
        e, o, m = l2(got[k], ref), outliers(got[k], ref, tol_g), scale_err(got[k], ref)
        if k.startswith("d."):
            w["l2t"], w["ot"] = max(w["l2t"], e), max(w["ot"], o)
        else:
            w["l2p"], w["op"] = max(w["l2p"], (e, k)), max(w["op"], (o, k))
        w["mx"] = max(w["mx"], (m, k))
    return GradErr(w["l2t"], w["ot"], w["l2p"][0], w["l2p"][1], w["op"][0], w["op"][1], w["mx"][0], w["mx"][1])


def fmt(e):
    return (f"L2: d tokens {e.l2_tokens:.2e} worst parameter {e.l2_name} {e.l2_param:.2e}; entries past tolerance: d tokens {e.out_tokens:.1e} "
            f"parameters {e.out_name} {e.out_param:.1e}")


def report_path():
    """parity_gpt_edges.txt in the directory the sibling GPU tests keep their parity reports in (test_transfuser_gpu.py::REPORT)."""
    from test_transfuser_gpu import REPORT as sibling
    return os.path.join(os.path.dirname(sibling), "parity_gpt_edges.txt")


def log(msg):
    path = report_path()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(msg + "\n")
