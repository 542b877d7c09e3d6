"""d loss / d image through the ViT encoders (include/mfvit.h, mfvit_vit_backward_ex): the patch-embedding data gradient stored straight into
the NCHW image by the col2im epilogue of the tile GEMM, and the data-gradient-only backward of a frozen backbone.

References: oracle.ref_vit / oracle.ref_fusion in float64 under torch autograd on the CPU.  Gates: measured on an MI355X, then fixed at >= 2 x
the measured error and never looser than the TOL of tests/test_vit_dropout_gpu.py (or 1e-5 for fp32)."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rng_tensor
from oracle import ref_fusion, ref_vit

DEV = "cuda:0"
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
# measured on one MI355X (largest over the tests of each precision): fp32 1.9e-6, bf16x3 4.6e-4, fp16 2.9e-3, bf16 1.6e-2
TOL = {"fp32": 1e-5, "bf16x3": 1e-3, "fp16": 1e-2, "bf16": 4e-2}
PROF_GEMM_TN = 3                                        # kernel class of the weight-gradient GEMMs (mfvit_prof_*)


def rel_err(got, ref):
    ref, got = ref.detach().double().cpu(), got.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def freeze_all_but_head(m):
    """The reference's fine-tune freezing loop (MAIN_CA:296-305): every parameter but the head's."""
    for name, p in m.named_parameters():
        if name not in ("head.weight", "head.bias"):
            p.requires_grad = False


def build(arch="vit_small", depth=12, precision="bf16x3", seed=7, img_size=224, **kw):
    import vits
    m = getattr(vits, arch)(num_classes=3, depth=depth, precision=precision, img_size=img_size, **kw)
    sd = ref_vit.seeded_params(seed, arch=arch, num_classes=3, depth=depth)
    sd["pos_embed"] = m.pos_embed.detach().clone()      # (the fixed sin-cos table of the model's own grid: non-square images too)
    m.load_state_dict(sd)
    return m.to(DEV), sd


def ref_img_grad(sd, img, y, frozen=(), heads=12, logits_fn=None):
    """float64 d CE(forward(img), y) / d img (and the logits, parameter dict) on the CPU."""
    pd = {k: v.double().requires_grad_(k != "pos_embed" and k not in frozen) for k, v in sd.items()}
    x = img.double().requires_grad_(True)
    logits = logits_fn(pd, x) if logits_fn else ref_vit.forward(pd, x, heads)
    F.cross_entropy(logits, y).backward()
    return x.grad, logits, pd


def prof_counts(fn):
    """Launches per kernel class (include/mfvit.h, mfvit_prof_*) of what fn() enqueues."""
    import ctypes
    from mfvit import _lib
    lib = _lib.lib()
    out = (ctypes.c_double * 40)()
    torch.cuda.synchronize()
    lib.mfvit_prof_collect(out, 10)                     # (clears stale records)
    lib.mfvit_prof_enable((1 << 10) - 1)
    try:
        fn()
        torch.cuda.synchronize()
        lib.mfvit_prof_collect(out, 10)
    finally:
        lib.mfvit_prof_enable(0)
    return [int(out[c * 4]) for c in range(10)]


# ------------------------------------------------------------------------------------------------ 1. trainable backbone, four precisions
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16", "fp16"])
def test_image_gradient_matches_float64(precision):
    B = 3
    m, sd = build(precision=precision)
    img = rng_tensor(51, (B, 3, 224, 224))
    y = torch.tensor([0, 2, 1])
    x = img.to(DEV).requires_grad_(True)
    F.cross_entropy(m(x), y.to(DEV)).backward()
    assert x.grad is not None and x.grad.shape == img.shape and x.grad.dtype == torch.float32
    gref, _, pd = ref_img_grad(sd, img, y)
    e = rel_err(x.grad, gref)
    print(f"[{precision}] d img rel err {e:.2e}")
    assert e < TOL[precision], e
    # the parameter gradients are still there (the same backward call formed both)
    eq = rel_err(m.blocks[0].attn.qkv.weight.grad, pd["blocks.0.attn.qkv.weight"].grad)
    assert eq < 4 * TOL[precision], eq


# ------------------------------------------------------------------------------------------------ 2. frozen backbone: data-gradient-only backward
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_frozen_backbone_forms_the_image_gradient_and_no_weight_gradient(mode):
    B = 3
    m, sd = build()
    freeze_all_but_head(m)
    getattr(m, mode)()
    img = rng_tensor(52, (B, 3, 224, 224))
    y = torch.tensor([2, 0, 1])
    x = img.to(DEV).requires_grad_(True)
    loss = F.cross_entropy(m(x), y.to(DEV))
    counts = prof_counts(loss.backward)
    assert counts[PROF_GEMM_TN] == 0, counts
    frozen = [n for n, _ in m.named_parameters() if not n.startswith("head.")]
    for name, p in m.named_parameters():
        assert (p.grad is None) == (name in frozen), name
    gref, _, pd = ref_img_grad(sd, img, y, frozen=frozen)
    e = rel_err(x.grad, gref)
    print(f"[frozen {mode}] d img rel err {e:.2e}")
    assert e < TOL["bf16x3"], e
    assert rel_err(m.head.weight.grad, pd["head.weight"].grad) < TOL["bf16x3"]
    # (the observable does see the weight gradients of a trainable backbone)
    m2, _ = build(depth=2)
    getattr(m2, mode)()
    loss2 = F.cross_entropy(m2(img.to(DEV)), y.to(DEV))
    assert prof_counts(loss2.backward)[PROF_GEMM_TN] > 0


@pytest.mark.gpu
def test_frozen_backbone_autograd_grad_and_double_backward_is_refused():
    from mfvit import _lib
    m, sd = build(depth=2)
    for p in m.parameters():
        p.requires_grad = False
    img = rng_tensor(53, (2, 3, 224, 224))
    y = torch.tensor([1, 0])
    x = img.to(DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(F.cross_entropy(m(x), y.to(DEV)), x)
    gref, _, _ = ref_img_grad(sd, img, y, frozen=list(sd))
    assert rel_err(g, gref) < TOL["bf16x3"]
    x2 = img.to(DEV).requires_grad_(True)
    with pytest.raises(_lib.MfvitError, match="create_graph"):
        torch.autograd.grad(F.cross_entropy(m(x2), y.to(DEV)), x2, create_graph=True)


# ------------------------------------------------------------------------------------------------ 3. no effect on the parameter gradients
@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 128])
def test_parameter_gradients_and_logits_are_bit_identical_with_an_image_gradient(B):
    m, _ = build()
    img = rng_tensor(54, (B, 3, 224, 224)).to(DEV)
    y = (torch.arange(B) % 3).to(DEV)
    runs = []
    for want in (False, True, False):
        m.zero_grad(set_to_none=True)
        x = img.clone().requires_grad_(want)
        logits = m(x)
        F.cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), [p.grad.clone() for p in m.parameters() if p.requires_grad], x.grad))
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0])
        assert len(r[1]) == len(runs[0][1]) > 100
        assert all(torch.equal(a, b) for a, b in zip(r[1], runs[0][1]))
    assert runs[0][2] is None and runs[1][2] is not None and torch.isfinite(runs[1][2]).all()


# ------------------------------------------------------------------------------------------------ 4. stop_grad_conv1, vit_base, non-square images
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["stop_grad_conv1", "vit_base", "non_square"])
def test_image_gradient_variants(case):
    B, size, depth = 3, (224, 224), 4
    if case == "stop_grad_conv1":
        depth = 12                                      # (the image and depth of test_image_gradient_matches_float64: the same d img bits, below)
        m, sd = build(depth=depth, stop_grad_conv1=True)
    elif case == "vit_base":
        B = 2
        m, sd = build(arch="vit_base", depth=depth)
        assert m.embed_dim == 768                       # (the unfused path: plain tile GEMMs + LayerNorm row passes)
    else:
        size = (224, 320)
        m, sd = build(depth=depth, img_size=size)
        assert m.num_tokens == 14 * 20 + 1
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert (case == "stop_grad_conv1") == ("patch_embed.proj.weight" in frozen)
    img = rng_tensor(51 if case == "stop_grad_conv1" else 55, (B, 3) + size)
    y = torch.tensor([0, 2, 1][:B])
    x = img.to(DEV).requires_grad_(True)
    F.cross_entropy(m(x), y.to(DEV)).backward()
    assert (m.patch_embed.proj.weight.grad is None) == (case == "stop_grad_conv1")
    gref, _, _ = ref_img_grad(sd, img, y, frozen=frozen)
    e = rel_err(x.grad, gref)
    print(f"[{case}] d img rel err {e:.2e}")
    assert e < TOL["bf16x3"], e
    if case == "stop_grad_conv1":                       # W_pe is frozen, not cut out: the image gradient is the trainable model's, bit for bit
        t, _ = build(depth=depth)
        xt = img.to(DEV).requires_grad_(True)
        F.cross_entropy(t(xt), y.to(DEV)).backward()
        assert t.patch_embed.proj.weight.grad is not None
        assert torch.equal(xt.grad, x.grad)


# ------------------------------------------------------------------------------------------------ 5. dropout / attention dropout / drop path
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16"])
@pytest.mark.parametrize("frozen", [False, True])
def test_image_gradient_in_training_mode_with_dropout(precision, frozen):
    from test_vit_dropout_gpu import masks_of, ref_logits
    B, depth = 3, 4
    m, sd = build(depth=depth, precision=precision, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.4)
    m.train()
    if frozen:
        freeze_all_but_head(m)
    img = rng_tensor(56, (B, 3, 224, 224))
    y = torch.tensor([1, 1, 0])
    x = img.to(DEV).requires_grad_(True)
    torch.manual_seed(13)
    logits = m(x)
    mk, rates = masks_of(m, B, m.num_tokens, 12)
    F.cross_entropy(logits, y.to(DEV)).backward()
    fz = [n for n, p in m.named_parameters() if not p.requires_grad]
    gref, _, _ = ref_img_grad(sd, img, y, frozen=fz, logits_fn=lambda pd, xx: ref_logits(pd, xx, 12, mk, rates))
    e = rel_err(x.grad, gref)
    print(f"[dropout {precision} frozen={frozen}] d img rel err {e:.2e}")
    assert e < TOL[precision], e


# ------------------------------------------------------------------------------------------------ 6. two-stream Fus_CrossViT (CA step)
def _ca(frozen, two_streams):
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    depth = 3
    vit_p = [ref_vit.seeded_params(17 + i, num_classes=3, depth=depth) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(19)
    backs = []
    for p in vit_p:
        b = vits.vit_small(num_classes=3, depth=depth)
        b.load_state_dict(p)
        b = b.to(DEV)
        if frozen:
            freeze_all_but_head(b)
        backs.append(b)
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    model = model.to(DEV)
    model._two_streams = two_streams
    return model, backs, vit_p, fus_p


@pytest.mark.gpu
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("two_streams", [True, False])
def test_fus_crossvit_image_gradients_match_float64(frozen, two_streams):
    from mfvit.losses import cross_entropy
    model, backs, vit_p, fus_p = _ca(frozen, two_streams)
    B = 2
    x, xe = rng_tensor(57, (B, 3, 224, 224)), rng_tensor(58, (B, 3, 224, 224))
    y = torch.tensor([2, 0])
    xc, xn = x.to(DEV).requires_grad_(True), xe.to(DEV).requires_grad_(True)
    fused, x_c, x_e = model(backs[0], backs[1], xc, xn)
    loss, _ = cross_entropy(fused + x_c + x_e, y.to(DEV))
    gc, ge = torch.autograd.grad(loss, (xc, xn))
    fpd = {k: v.double().requires_grad_(True) for k, v in fus_p.items()}
    vpd = [{k: v.double().requires_grad_(k != "pos_embed") for k, v in p.items()} for p in vit_p]
    xr, xer = x.double().requires_grad_(True), xe.double().requires_grad_(True)
    _, _, r_loss, _ = ref_fusion.ca_step(fpd, vpd[0], vpd[1], xr, xer, y)
    rc, re_ = torch.autograd.grad(r_loss, (xr, xer))
    ec, ee = rel_err(gc, rc), rel_err(ge, re_)
    print(f"[CA frozen={frozen} two={two_streams}] d img_cxr {ec:.2e}, d img_enh {ee:.2e}")
    assert ec < TOL["bf16x3"] and ee < TOL["bf16x3"], (ec, ee)
    if frozen:
        for b in backs:
            assert all(p.grad is None for p in b.parameters())


# ------------------------------------------------------------------------------------------------ 7. reproducible image gradient
@pytest.mark.gpu
def test_image_gradient_is_the_same_bits_over_two_runs():
    B = 128
    m, _ = build()
    img = rng_tensor(59, (B, 3, 224, 224)).to(DEV)
    y = (torch.arange(B) % 3).to(DEV)
    out = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        x = img.clone().requires_grad_(True)
        F.cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        out.append(x.grad.clone())
    assert torch.equal(out[0], out[1])
    assert float(out[0].abs().max()) > 0
