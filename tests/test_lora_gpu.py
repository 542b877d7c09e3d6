"""LoRA adapters on the ViT encoders (mfvit.lora; include/mfvit.h: mfvit_vit_prepare_shadow_lora, mfvit_vit_backward_lora,
mfvit_vit_lora_grad) against float64: oracle.ref_vit / oracle.ref_fusion on the merged parameter dict of tests/lora_ref.py, the adapters'
gradients by torch autograd through it.  B = 3, 224 x 224, seeded nonzero A and B, every B scaled so that max|s B A| = 2^-6 max|W|.

Gates.  Logits: TOL of tests/test_input_grad_gpu.py.  Gradients, max-norm relative error per tensor: GRAD_GATE, fixed at >= 2 x the
largest error measured on one MI355X and never looser than 4 TOL (the bound test_input_grad_gpu.py uses for qkv.weight.grad).
Measured (largest over the tensors of a test):
  bf16x3  depth 12 default targets 5.3e-4 | blocks [2, 3] of 4 4.5e-4 | all six, depth 2: vit_small 6.1e-4, vit_base 7.6e-4 | beside trainable
          LayerNorms 6.3e-4 (the norms 3.9e-4) | Fus_CrossViT 4.6e-4 (fusion parameters 1.8e-5) | drop path 4.6e-4      -> gate 2e-3
  fp32    depth 12 default targets 9.4e-6 | all six, depth 2, rank 3 2.6e-6                                              -> gate 2.5e-5
  logits  bf16x3 1.6e-5, fp32 3.8e-6;  d img with adapters 2.8e-4;  head gradients 1.3e-5 / 2.0e-6
  small update (2^-8 max|W|): 1.73e-3 of the update's effect on the logits, against a split-bf16 floor of 5.64e-4 (gate 4 x = 2.26e-3)"""
import importlib

import pytest
import torch
import torch.nn.functional as F

import lora_ref
from conftest import rng_tensor
from oracle import ref_fusion, ref_vit
from test_input_grad_gpu import DEV, FUS_MOD, PROF_GEMM_TN, TOL, build, prof_counts, rel_err

pytestmark = pytest.mark.gpu
GRAD_GATE = {"bf16x3": 2e-3, "fp32": 2.5e-5}
assert all(GRAD_GATE[p] <= 4 * TOL[p] for p in GRAD_GATE)
HEADS = 12
Y3 = torch.tensor([0, 2, 1])


def attach(m, sd, rank=8, alpha=16.0, targets=("q", "v"), blocks=None, seed=31, ratio=2.0 ** -6, freeze_base=True):
    """add_lora + seeded nonzero adapters (lora_ref.seeded_adapters) loaded into them: (adapter tensors, s, block list)."""
    from mfvit import lora
    lora.add_lora(m, rank=rank, alpha=alpha, targets=targets, blocks=blocks, freeze_base=freeze_base)
    blks = list(range(m.depth)) if blocks is None else sorted(b % m.depth for b in blocks)
    s = alpha / rank
    ad = lora_ref.seeded_adapters(seed, sd, rank, blks, targets, s, ratio)
    lora.load_lora_state_dict(m, ad)
    return ad, s, blks


def ref_step(sd, ad, s, blks, targets, img, y, train=("head.weight", "head.bias"), logits_fn=None, want_img=False):
    """float64 CE step on the merged dict: (logits, parameter dict, adapter dict, image) with .grad on what requires it."""
    pd = {k: v.double().requires_grad_(k in train) for k, v in sd.items()}
    adg = {k: v.double().requires_grad_(True) for k, v in ad.items()}
    x = img.double().requires_grad_(want_img)
    mp = lora_ref.merged(pd, adg, s, blks, targets)
    logits = logits_fn(mp, x) if logits_fn else ref_vit.forward(mp, x, HEADS)
    F.cross_entropy(logits, y).backward()
    return logits, pd, adg, x


def adapter_errors(m, adg):
    named = dict(m.named_parameters())
    errs = {}
    for k, v in adg.items():
        assert named[k].grad is not None and named[k].grad.shape == v.shape, k
        errs[k] = rel_err(named[k].grad, v.grad)
    return errs


def worst(errs):
    k = max(errs, key=errs.get)
    return k, errs[k]


def arena_grads_are_none(m):
    return all(p.grad is None for _, p in m.arena_named_parameters())


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_logits_match_the_oracle_on_the_merged_weights(precision):
    m, sd = build(precision=precision)
    ad, s, blks = attach(m, sd)
    img = rng_tensor(61, (3, 3, 224, 224))
    with torch.no_grad():
        logits = m(img.to(DEV))
        pd = {k: v.double() for k, v in sd.items()}
        ref = ref_vit.forward(lora_ref.merged(pd, ad, s, blks, ("q", "v")), img.double(), HEADS)
        base = ref_vit.forward(pd, img.double(), HEADS)
    e = rel_err(logits, ref)
    print(f"[{precision}] adapted logits rel err {e:.2e}; the adapters move the logits by {rel_err(ref, base):.2e}")
    assert rel_err(ref, base) > 10 * TOL[precision]          # (the adapters matter at this tolerance)
    assert e < TOL[precision], e


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_fresh_adapters_leave_the_logits_bit_identical(precision):
    from mfvit import lora
    m, _ = build(depth=3, precision=precision)
    img = rng_tensor(62, (3, 3, 224, 224)).to(DEV)
    with torch.no_grad():
        before = m(img).clone()
        lora.add_lora(m, targets=lora.TARGETS)               # B = 0
        after = m(img).clone()
    assert m._lora.eff is not None
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))


def test_a_small_update_is_resolved_by_the_default_precision():
    """max|s B A| = 2^-8 max|W|: logits_adapted - logits_base against the oracle's.  Gate: 4 x the floor of the split-bf16 grid, from the
    reference alone (lora_ref.split_floor: the float64 oracle with the merged weights rounded to hi + lo, against unrounded).  A plain
    16-bit shadow misses it by an order of magnitude."""
    from mfvit import lora
    m, sd = build()
    img = rng_tensor(61, (3, 3, 224, 224))
    with torch.no_grad():
        base = m(img.to(DEV)).double().cpu()
    ad, s, blks = attach(m, sd, ratio=2.0 ** -8)
    floor, d_ref = lora_ref.split_floor(sd, ad, s, blks, ("q", "v"), img)
    with torch.no_grad():
        d = m(img.to(DEV)).double().cpu() - base
    e = float((d - d_ref).abs().max() / d_ref.abs().max())
    print(f"small update: |d - d_ref| / |d_ref| = {e:.2e}, split-bf16 floor {floor:.2e} (gate 4 x), max|d_ref| {float(d_ref.abs().max()):.2e}")
    assert lora.has_lora(m)
    assert e <= 4 * floor, (e, floor)


# ------------------------------------------------------------------------------------------------ backward, base frozen
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_adapter_and_head_gradients_match_float64_with_one_weight_gradient_launch_per_block(precision):
    m, sd = build(precision=precision)
    ad, s, blks = attach(m, sd)
    img = rng_tensor(63, (3, 3, 224, 224))
    loss = F.cross_entropy(m(img.to(DEV)), Y3.to(DEV))
    counts = prof_counts(loss.backward)
    assert counts[PROF_GEMM_TN] == m.depth, counts            # the fused qkv weight gradient of every block, nothing else
    _, pd, adg, _ = ref_step(sd, ad, s, blks, ("q", "v"), img, Y3)
    errs = adapter_errors(m, adg)
    k, e = worst(errs)
    eh = rel_err(m.head.weight.grad, pd["head.weight"].grad)
    print(f"[{precision}] depth 12 default targets: worst adapter grad rel err {e:.2e} ({k}), head {eh:.2e}")
    assert len(errs) == 12 * 4
    assert e < GRAD_GATE[precision], (k, e)
    assert eh < TOL[precision] and rel_err(m.head.bias.grad, pd["head.bias"].grad) < TOL[precision]
    assert arena_grads_are_none(m)


def test_launch_census_without_adapters_and_for_all_six_targets():
    from mfvit import lora
    img = rng_tensor(64, (3, 3, 224, 224)).to(DEV)

    def tn_launches(m):
        return prof_counts(F.cross_entropy(m(img), Y3.to(DEV)).backward)[PROF_GEMM_TN]
    m, sd = build(depth=2)
    attach(m, sd, targets=lora.TARGETS)
    six = tn_launches(m)
    lora.remove_lora(m)
    for _, p in m.arena_named_parameters():
        p.requires_grad_(False)
    assert tn_launches(m) == 0                                # adapters removed, base frozen: no weight gradient at all
    full, _ = build(depth=2)
    n_full = tn_launches(full)
    print(f"weight-gradient launches at depth 2: all six targets {six}, full fine-tune {n_full}")
    assert 0 < six < n_full


def test_partial_depth_forms_no_weight_gradient_below_the_lowest_adapted_block():
    m, sd = build(depth=4)
    ad, s, blks = attach(m, sd, blocks=[2, 3])
    assert blks == [2, 3]
    img = rng_tensor(65, (3, 3, 224, 224))
    loss = F.cross_entropy(m(img.to(DEV)), Y3.to(DEV))
    counts = prof_counts(loss.backward)
    assert counts[PROF_GEMM_TN] == 2, counts
    _, pd, adg, _ = ref_step(sd, ad, s, blks, ("q", "v"), img, Y3)
    k, e = worst(adapter_errors(m, adg))
    print(f"blocks [2, 3] of 4: worst adapter grad rel err {e:.2e} ({k})")
    assert e < GRAD_GATE["bf16x3"], (k, e)
    assert not any("lora_" in n and n.startswith(("blocks.0.", "blocks.1.")) for n, _ in m.named_parameters())
    assert arena_grads_are_none(m)


@pytest.mark.parametrize("arch,rank,precision", [("vit_small", 8, "bf16x3"), ("vit_small", 3, "fp32"), ("vit_base", 8, "bf16x3")])
def test_all_six_targets_match_float64(arch, rank, precision):
    from mfvit import lora
    m, sd = build(arch=arch, depth=2, precision=precision)
    ad, s, blks = attach(m, sd, rank=rank, alpha=2.0 * rank, targets=lora.TARGETS)
    img = rng_tensor(66, (3, 3, 224, 224))
    F.cross_entropy(m(img.to(DEV)), Y3.to(DEV)).backward()
    logits, pd, adg, _ = ref_step(sd, ad, s, blks, lora.TARGETS, img, Y3)
    errs = adapter_errors(m, adg)
    k, e = worst(errs)
    print(f"[{arch} r={rank} {precision}] all six targets: worst adapter grad rel err {e:.2e} ({k})")
    assert len(errs) == 2 * 6 * 2
    assert e < GRAD_GATE[precision], (k, e)
    assert arena_grads_are_none(m)


def test_adapters_beside_trainable_layernorms():
    """Base arena parameters that require a gradient: the full backward, then the contraction of the adapted dW slices of its arena."""
    from mfvit import lora
    img = rng_tensor(67, (3, 3, 224, 224))
    norms = [f"blocks.{i}.norm{j}.{w}" for i in range(2) for j in (1, 2) for w in ("weight", "bias")]

    def run(with_adapters, zero_b):
        m, sd = build(depth=2)
        ad = s = blks = None
        if with_adapters:
            ad, s, blks = attach(m, sd)
            if zero_b:
                with torch.no_grad():
                    for n, p in m.named_parameters():
                        if "lora_B" in n:
                            p.zero_()
        named = dict(m.named_parameters())
        for n, p in named.items():
            if "lora_" not in n and not n.startswith("head."):
                p.requires_grad_(n in norms)
        F.cross_entropy(m(img.to(DEV)), Y3.to(DEV)).backward()
        torch.cuda.synchronize()
        return m, sd, ad, s, blks
    m, sd, ad, s, blks = run(True, False)
    _, pd, adg, _ = ref_step(sd, ad, s, blks, ("q", "v"), img, Y3, train=tuple(norms) + ("head.weight", "head.bias"))
    k, e = worst(adapter_errors(m, adg))
    named = dict(m.named_parameters())
    en = max(rel_err(named[n].grad, pd[n].grad) for n in norms)
    print(f"mixed: worst adapter grad rel err {e:.2e} ({k}), worst norm grad {en:.2e}")
    assert e < GRAD_GATE["bf16x3"] and en < GRAD_GATE["bf16x3"], (k, e, en)
    assert named["blocks.0.attn.qkv.weight"].grad is None
    # B = 0: the arena gradients are the bits of the same model without adapters
    m0 = run(True, True)[0]
    m1 = run(False, False)[0]
    n0, n1 = dict(m0.named_parameters()), dict(m1.named_parameters())
    for n in norms + ["head.weight", "head.bias"]:
        assert torch.equal(n0[n].grad.view(torch.int32), n1[n].grad.view(torch.int32)), n


def test_image_gradient_with_adapters_and_unchanged_adapter_gradients():
    m, sd = build()
    ad, s, blks = attach(m, sd)
    img = rng_tensor(68, (3, 3, 224, 224))
    got = []
    for want in (False, True):
        m.zero_grad(set_to_none=True)
        x = img.to(DEV).requires_grad_(want)
        F.cross_entropy(m(x), Y3.to(DEV)).backward()
        torch.cuda.synchronize()
        got.append(([p.grad.clone() for n, p in m.named_parameters() if "lora_" in n], x.grad))
    _, _, adg, xr = ref_step(sd, ad, s, blks, ("q", "v"), img, Y3, want_img=True)
    e = rel_err(got[1][1], xr.grad)
    print(f"d img with adapters rel err {e:.2e}")
    assert got[0][1] is None and e < TOL["bf16x3"], e         # the gate of test_image_gradient_matches_float64
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    k, ea = worst(adapter_errors(m, adg))
    assert ea < GRAD_GATE["bf16x3"], (k, ea)
    assert arena_grads_are_none(m)


# ------------------------------------------------------------------------------------------------ merge, remove, optimizer step
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_merge_keeps_the_logits_bits_and_remove_restores_the_base(precision):
    from mfvit import lora
    img = rng_tensor(69, (3, 3, 224, 224)).to(DEV)
    m, sd = build(depth=3, precision=precision)
    keys = set(m.state_dict().keys())
    arena0 = m.flat_parameters().clone()
    with torch.no_grad():
        base = m(img).clone()
        attach(m, sd, targets=lora.TARGETS)
        adapted = m(img).clone()
        assert not torch.equal(adapted, base)
        assert torch.equal(m.flat_parameters().view(torch.int32), arena0.view(torch.int32))      # the arena is never written while attached
        lora.merge_lora(m)
        merged = m(img).clone()
    assert torch.equal(merged.view(torch.int32), adapted.view(torch.int32))
    assert set(m.state_dict().keys()) == keys and not lora.has_lora(m)
    assert not torch.equal(m.flat_parameters(), arena0)
    m2, sd2 = build(depth=3, precision=precision)
    with torch.no_grad():
        attach(m2, sd2, targets=lora.TARGETS)
        assert torch.equal(m2(img).view(torch.int32), adapted.view(torch.int32))
        lora.remove_lora(m2)
        assert torch.equal(m2(img).view(torch.int32), base.view(torch.int32))
    assert torch.equal(m2.flat_parameters().view(torch.int32), arena0.view(torch.int32))


def test_an_optimizer_step_on_the_adapters_reaches_the_next_forward():
    from mfvit import lora
    from mfvit.optim import AdamW
    m, _ = build(depth=3)
    lora.add_lora(m)                                          # B = 0
    img = rng_tensor(70, (3, 3, 224, 224)).to(DEV)
    arena0 = m.flat_parameters().clone()
    opt = AdamW(lora.lora_parameters(m), lr=1e-2, weight_decay=0.0)
    first = m(img)
    F.cross_entropy(first, Y3.to(DEV)).backward()
    opt.step()
    torch.cuda.synchronize()
    assert any(float(p.detach().abs().max()) > 0 for n, p in m.named_parameters() if "lora_B" in n)
    assert torch.equal(m.flat_parameters().view(torch.int32), arena0.view(torch.int32))
    with torch.no_grad():
        second = m(img)
        feats_a = m.features3D(img)                           # features3D then __call__ on one tensor: the single-use feature cache
        third = m(img)
    assert not torch.equal(second, first.detach())            # the shadow key saw the adapters' versions
    assert torch.equal(third, second) and torch.equal(m.forward_head(feats_a), second)
    with torch.no_grad():
        for p in lora.lora_parameters(m):
            p.mul_(0.5)
        assert not torch.equal(m(img), second)                # ... and so does the feature cache's key, straight after a cached pair


@pytest.mark.parametrize("B", [3, 16])
def test_adapter_gradients_are_the_same_bits_over_two_backwards(B):
    m, sd = build(depth=3)
    attach(m, sd, targets=("q", "v", "fc1"))
    img = rng_tensor(71, (B, 3, 224, 224)).to(DEV)
    y = (torch.arange(B) % 3).to(DEV)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        F.cross_entropy(m(img), y).backward()
        torch.cuda.synchronize()
        runs.append([p.grad.clone() for n, p in m.named_parameters() if "lora_" in n])
    assert len(runs[0]) == 3 * 3 * 2
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ two-stream model, drop path
def test_fus_crossvit_with_adapters_on_both_backbones():
    import vits_returnftrs as vits
    from mfvit import lora
    from mfvit.losses import cross_entropy
    fus = importlib.import_module(FUS_MOD)
    depth, B = 2, 2
    vit_p = [ref_vit.seeded_params(17 + i, num_classes=3, depth=depth) for i in range(2)]
    fus_p = ref_fusion.seeded_fusion_params(19)
    backs, ads = [], []
    for i, p in enumerate(vit_p):
        b = vits.vit_small(num_classes=3, depth=depth)
        b.load_state_dict(p)
        b = b.to(DEV)
        ads.append(attach(b, p, seed=40 + i))
        backs.append(b)
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(fus_p)
    model = model.to(DEV)
    x, xe = rng_tensor(72, (B, 3, 224, 224)), rng_tensor(73, (B, 3, 224, 224))
    y = torch.tensor([2, 0])
    fused, x_c, x_e = model(backs[0], backs[1], x.to(DEV), xe.to(DEV))
    loss, _ = cross_entropy(fused + x_c + x_e, y.to(DEV))
    loss.backward()
    fpd = {k: v.double().requires_grad_(True) for k, v in fus_p.items()}
    vpd = [{k: v.double().requires_grad_(k.startswith("head.")) for k, v in p.items()} for p in vit_p]
    adg = [{k: v.double().requires_grad_(True) for k, v in ad.items()} for ad, _, _ in ads]
    mp = [lora_ref.merged(vpd[i], adg[i], ads[i][1], ads[i][2], ("q", "v")) for i in range(2)]
    r_out, _, r_loss, _ = ref_fusion.ca_step(fpd, mp[0], mp[1], x.double(), xe.double(), y)
    r_loss.backward()
    e_out = rel_err(fused + x_c + x_e, r_out)
    errs = [worst(adapter_errors(backs[i], adg[i])) for i in range(2)]
    named = dict(model.named_parameters())
    ef = max(rel_err(named[k].grad, v.grad) for k, v in fpd.items() if v.grad is not None and float(v.grad.abs().max()) > 0)
    print(f"CA with adapters: logits {e_out:.2e}, adapter grads {errs[0][1]:.2e} / {errs[1][1]:.2e}, worst fusion grad {ef:.2e}")
    assert e_out < TOL["bf16x3"]
    assert errs[0][1] < GRAD_GATE["bf16x3"] and errs[1][1] < GRAD_GATE["bf16x3"], errs
    assert ef < GRAD_GATE["bf16x3"], ef
    assert all(arena_grads_are_none(b) for b in backs) and lora.has_lora(backs[0])


def test_drop_path_gradients_match_the_reference_with_the_exported_masks():
    from test_vit_dropout_gpu import masks_of, ref_logits
    import vits
    depth, B = 3, 3
    m = vits.vit_small(num_classes=3, depth=depth, drop_path_rate=0.2)
    sd = ref_vit.seeded_params(7, num_classes=3, depth=depth)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    ad, s, blks = attach(m, sd, targets=("q", "v", "fc2"))
    img = rng_tensor(74, (B, 3, 224, 224))
    torch.manual_seed(5)
    loss = F.cross_entropy(m(img.to(DEV)), Y3.to(DEV))
    mk, rates = masks_of(m, B, m.num_tokens, HEADS)
    assert any(k[0] == "dp_attn" for k in mk if isinstance(k, tuple))
    loss.backward()
    _, pd, adg, _ = ref_step(sd, ad, s, blks, ("q", "v", "fc2"), img, Y3, logits_fn=lambda p, x: ref_logits(p, x, HEADS, mk, rates))
    k, e = worst(adapter_errors(m, adg))
    print(f"drop path 0.2: worst adapter grad rel err {e:.2e} ({k})")
    assert e < GRAD_GATE["bf16x3"], (k, e)
    assert arena_grads_are_none(m)


# ------------------------------------------------------------------------------------------------ C ABI of the encoder entries
def test_encoder_entries_return_einval_before_any_launch():
    """Every buffer has its full size, so that a request accepted by mistake would still stay inside them."""
    import ctypes
    from mfvit import _lib, lora
    lib = _lib.lib()
    m, sd = build(depth=2)
    attach(m, sd)
    img = rng_tensor(75, (2, 3, 224, 224)).to(DEV)
    cfg = m._cfg(img, True)
    arena = m.flat_parameters()
    eff, dw = torch.empty_like(arena), torch.empty_like(arena)
    shadow = torch.empty(lib.mfvit_vit_shadow_bytes(cfg), device=DEV, dtype=torch.uint8)
    ws = torch.empty(lib.mfvit_vit_workspace_bytes(cfg), device=DEV, dtype=torch.uint8)
    dfe = torch.zeros(2, m.num_tokens, m.embed_dim, device=DEV)
    lo = m._lora
    grads = lo.new_grads(DEV)
    st = torch.cuda.current_stream().cuda_stream
    before = eff.clone()

    def prep(cfg_=cfg, req=None, params=arena.data_ptr(), eff_=eff.data_ptr()):
        return lib.mfvit_vit_prepare_shadow_lora(cfg_, params, req, eff_, shadow.data_ptr(), st)

    def bwd(cfg_=cfg, req=None, dw_=dw.data_ptr(), hi=2, lo_=0, dimg=None):
        return lib.mfvit_vit_backward_lora(cfg_, None, eff.data_ptr(), shadow.data_ptr(), ws.data_ptr(), dfe.data_ptr(), req, dw_, dimg, hi, lo_, st)

    def edited(**kw):
        req = lo.request(grads=grads)
        keep = req._keep
        for k, v in kw.items():
            if k in ("rank", "n", "scale"):
                setattr(req, k, v)
            else:                                   # a field of item 0
                setattr(req.items[0], k, v)
        req._keep = keep
        return req
    bad = [edited(rank=0), edited(rank=65), edited(n=0), edited(n=13), edited(block=2), edited(block=-1), edited(target=6), edited(target=-1),
           edited(a=None), edited(b=None), edited(block=1, target=0)]          # (the last: block 1 / q twice)
    for req in bad:
        assert prep(req=req) == -22 and bwd(req=req) == -22 and lib.mfvit_vit_lora_grad(cfg, req, dw.data_ptr(), st) == -22
    assert prep(req=None) == -22 and bwd(req=None) == -22                      # no request at all
    for req in (edited(da=None), edited(db=None)):                             # the gradient outputs: the two backward entries only
        assert bwd(req=req) == -22 and lib.mfvit_vit_lora_grad(cfg, req, dw.data_ptr(), st) == -22
    good = lo.request(grads=grads)
    assert prep(req=good, eff_=None) == -22 and prep(req=good, eff_=arena.data_ptr()) == -22 and prep(req=good, params=None) == -22
    assert bwd(req=good, dw_=None) == -22 and bwd(req=good, hi=1) == -22 and bwd(req=good, lo_=1) == -22 and bwd(req=good, lo_=-2) == -22
    assert lib.mfvit_vit_lora_grad(cfg, good, None, st) == -22
    tok = _lib.VitCfg.from_buffer_copy(cfg)
    tok.token_input, tok.tokens = 1, 197
    assert prep(cfg_=tok, req=good) == -22 and bwd(cfg_=tok, req=good) == -22
    nosave = _lib.VitCfg.from_buffer_copy(cfg)
    nosave.save_for_backward = 0
    assert bwd(cfg_=nosave, req=good) == -22
    torch.cuda.synchronize()
    assert torch.equal(eff.view(torch.int32), before.view(torch.int32))        # nothing was launched
    assert ctypes.sizeof(_lib.LoraItem) == 40 and lora.TARGETS.index("fc2") == 5


# ------------------------------------------------------------------------------------------------ what goes through _ensure_shadow
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_attention_maps_and_relevance_see_the_adapted_weights(precision):
    """No code of their own: the maps of a model with adapters are, bit for bit, the maps of the model with the adapters merged ('fp32' reads
    its weights from the arena the entry points are given: the effective one)."""
    from mfvit import lora
    img = rng_tensor(76, (2, 3, 224, 224)).to(DEV)
    m, sd = build(depth=3, precision=precision)
    base = m.get_attention_maps(img, blocks=[2], head_fusion="mean")[0].clone()
    attach(m, sd, targets=lora.TARGETS)
    maps = m.get_attention_maps(img, blocks=[2], head_fusion="mean")[0].clone()
    roll = m.attention_rollout(img).clone()
    rel = m.attention_relevance(img, target=1).clone() if precision == "bf16x3" else None
    assert not torch.equal(maps, base)
    lora.merge_lora(m)
    assert torch.equal(m.get_attention_maps(img, blocks=[2], head_fusion="mean")[0].view(torch.int32), maps.view(torch.int32))
    assert torch.equal(m.attention_rollout(img).view(torch.int32), roll.view(torch.int32))
    if rel is not None:
        assert torch.equal(m.attention_relevance(img, target=1).view(torch.int32), rel.view(torch.int32))
