"""GPU tests of patch dropout (timm PatchDropout) in the ViT encoders: the front end on the kept patches (csrc/patch_drop.hip) and the block
stack on the shortened sequence (mfvit_vit_forward_x0 / _backward_x0), against the float64 restatement tests/patch_drop_ref.py on the inputs
that file fixes (CASES; tests/test_patch_drop_cpu.py bounds the restatement's own float32 error on them).  Gates: patch_drop_ref.CAPS, the ones
the project applies to the undropped encoder in each precision.  Measured errors are printed (run with -s) and appended to the file MFVIT_PARITY_REPORT names."""
import ctypes
import importlib
import os

import pytest
import torch

import patch_drop_ref as R
from fusion_edges_ref import GATES as FUSION_GATES
from mfvit import _lib
from mfvit._lib import MfvitError
from oracle import ref_fusion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["fp32", "bf16x3", "bf16", "fp16"]
REPORT = os.environ.get("MFVIT_PARITY_REPORT")      # a file the measured figures are appended to (they are printed either way)
FUS_MOD = ("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
           "changemodelinputlocation_std002_sum")


def log(msg):
    print(msg)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")


def build(p, hw, depth, precision, **kw):
    import vits
    m = vits.vit_small(num_classes=3, depth=depth, precision=precision, img_size=hw, **kw)
    m.load_state_dict(p, strict=True)
    return m.to(DEV).train()


def run_case(name, precision, stop_grad_conv1=False, frozen=False):
    """The model's features, logits and gradients on a case of patch_drop_ref.CASES, checked against its float64 reference."""
    hw, depth, B, K, _, with_grads = R.CASES[name]
    p, img, idx, r, rl = R.case_inputs(name)
    ref = R.reference(name)
    m = build(p, hw, depth, precision, stop_grad_conv1=stop_grad_conv1)
    if frozen:
        for prm in m.parameters():
            prm.requires_grad_(False)
    x = img.to(DEV).requires_grad_(with_grads)
    ig = idx.to(DEV)
    cap_f, cap_g = R.CAPS[precision]
    with torch.set_grad_enabled(with_grads):
        f = m.features3D(x, keep_indices=ig)
        logits = m(x, keep_indices=ig)
    assert f.shape == (B, 1 + K, 384) and f.dtype == torch.float32
    assert torch.equal(m.last_keep_indices, ig)
    e_f, e_l = R.scale_err(f, ref["features"]), R.scale_err(logits, ref["logits"])
    msg = f"{name}[{precision},sgc1={int(stop_grad_conv1)},frozen={int(frozen)}] features {e_f:.2e} logits {e_l:.2e}"
    worst, e_d = ("", 0.0), 0.0
    if with_grads:
        ((f * r.to(DEV)).sum() + (logits * rl.to(DEV)).sum()).backward()
        for pname, prm in m.named_parameters():
            if frozen or pname == "pos_embed" or (stop_grad_conv1 and pname.startswith("patch_embed")):
                assert prm.grad is None, pname
                continue
            assert prm.grad is not None, pname
            e = R.scale_err(prm.grad, ref["grads"][pname])
            if e > worst[1]:
                worst = (pname, e)
        e_d = R.scale_err(x.grad, ref["dimg"])
        msg += f" worst grad {worst[0]} {worst[1]:.2e} dimg {e_d:.2e}"
        dropped = R.dropped_mask(idx, hw).expand(B, 3, hw[0], hw[1])
        assert bool((x.grad.cpu()[dropped] == 0.0).all()), "dropped patches of d img must be exact zeros"
    log(msg)
    m.check_keep_error()
    assert e_f < cap_f and e_l < cap_f, msg
    assert worst[1] < cap_g and e_d < cap_g, msg
    if precision == "fp32":
        assert logits.argmax(1).cpu().tolist() == ref["logits"].argmax(1).tolist()


# every shape of CASES in every precision: features, logits, all parameter gradients and d img where the case has gradients
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_features_logits_and_gradients_match_the_restatement(name, precision):
    run_case(name, precision)


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", ["sq64", "rect96x64", "sq64_ordered"])
def test_gradients_with_stop_grad_conv1(name, precision):
    run_case(name, precision, stop_grad_conv1=True)


@pytest.mark.parametrize("precision", MODES)
def test_frozen_backbone_returns_the_image_gradient_only(precision):
    run_case("rect96x64", precision, frozen=True)


def test_the_cases_straddle_every_attention_family_switch():
    """The B = 43 cases of patch_drop_ref.CASES sit on both sides of every switch of kernel family that mfvit_attention_plan reports between
    T = 2 and 197; at B = 2 / 3 it reports none."""
    lib = _lib.lib()

    def switches(dtype, B, backward):
        out, prev = [], None
        for T in range(2, 198):
            plan = (ctypes.c_int32 * 8)()
            assert lib.mfvit_attention_plan(dtype, B, T, 12, 32, backward, plan) == 0
            if prev is not None and plan[0] != prev:
                out.append(T)
            prev = plan[0]
        return out
    covered = {1 + c[3] for c in R.CASES.values() if c[2] == 43}
    for dtype in (_lib.F32, _lib.BF16, _lib.F16, _lib.X3F16):
        for backward in (0, 1):
            assert switches(dtype, 2, backward) == [] and switches(dtype, 3, backward) == []
            for T in switches(dtype, 43, backward):
                assert {T - 1, T} <= covered, (dtype, backward, T)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_a_sample_does_not_depend_on_its_batch(precision):
    """Sample b alone and inside a batch with other images and other indices: the same bits - the features in both precisions, the d img slice in
    the default bf16x3.  Finding (fp32, d img): the UNCHANGED fp32 data-gradient chain of the block stack is not bit-stable against the batch
    around a sample - measured on the full-grid encoder without patch dropout, alone against inside B = 3 at 96 x 64, depth 2: d img differs by
    4.6e-07 .. 6.7e-07 of its scale for samples 1 and 2 (sample 0, whose rows keep their place, is bit-equal); under patch dropout the d x_0 the
    front end is handed differs by 6.0e-07 .. 1.0e-06 in the same way and d img by 4.7e-07 .. 5.0e-07.  Existing kernels are out of this change's
    reach, so in fp32 the d img slice is held to 1e-5 (the figure tests/test_encoder_gpu.py uses for one backward in two summation orders) and the
    front end's own bit-stability is shown on equal d x_0 by test_front_end_is_bit_stable_against_the_batch."""
    hw, depth, B, K = (96, 64), 2, 3, 11
    p, img, idx, r, _ = R.case_inputs("rect96x64")
    m = build(p, hw, depth, precision)

    def go(sel):
        x = img[sel].contiguous().to(DEV).requires_grad_(True)
        f = m.features3D(x, keep_indices=idx[sel].to(DEV))
        (f * r[sel].to(DEV)).sum().backward()
        return f.detach(), x.grad.detach()
    f_all, d_all = go(slice(0, B))
    for b in range(B):
        f_b, d_b = go(slice(b, b + 1))
        assert torch.equal(f_all[b:b + 1], f_b), b
        if precision == "fp32":
            e = R.scale_err(d_all[b:b + 1], d_b)
            print(f"fp32 d img of sample {b}, alone vs in the batch: {e:.2e}")
            assert e < 1e-5, (b, e)
        else:
            assert torch.equal(d_all[b:b + 1], d_b), b


@pytest.mark.parametrize("precision", MODES)
def test_front_end_is_bit_stable_against_the_batch(precision):
    """mfvit_patch_keep_embed / _bwd called directly: x0 and, from the SAME d x0 rows, d img of sample b are the same bits alone and inside
    a batch with other images and indices, in every precision."""
    from mfvit._lib import check, lib, ptr, stream
    hw, depth, B, K = (96, 64), 1, 3, 11
    p, img, idx, _, _ = R.case_inputs("rect96x64")
    m = build(p, hw, 2, precision)
    dx0 = R.rng(9201, (B, 1 + K, 384)).to(DEV)
    img, idx = img.to(DEV), idx.to(DEV)
    a, off = m._arena.data_ptr(), m._offsets
    err = torch.zeros(1, device=DEV, dtype=torch.int32)

    def front_end(sel):
        im, ix, dx = img[sel].contiguous(), idx[sel].contiguous(), dx0[sel].contiguous()
        n = im.shape[0]
        pk = _lib.PatchKeepCfg(_lib.dtype_code(precision), n, hw[0], hw[1], K, 384)
        ws = torch.empty(lib().mfvit_patch_keep_workspace_bytes(pk, 1), device=DEV, dtype=torch.uint8)
        x0, dimg = torch.empty(n, 1 + K, 384, device=DEV), torch.empty_like(im)
        check(lib().mfvit_patch_keep_embed(pk, ptr(im), ptr(ix), a + 4 * off["cls_token"][0], a + 4 * off["pos_embed"][0],
                                           a + 4 * off["patch_embed.proj.weight"][0], a + 4 * off["patch_embed.proj.bias"][0], ptr(ws), 1, ptr(x0),
                                           ptr(err), stream()), "mfvit_patch_keep_embed")
        check(lib().mfvit_patch_keep_embed_bwd(pk, ptr(ix), ptr(ws), ptr(dx), None, None, None, ptr(dimg), ptr(err), stream()),
              "mfvit_patch_keep_embed_bwd")
        return x0, dimg
    x_all, d_all = front_end(slice(0, B))
    for b in range(B):
        x_b, d_b = front_end(slice(b, b + 1))
        assert torch.equal(x_all[b:b + 1], x_b) and torch.equal(d_all[b:b + 1], d_b), b
    assert int(err.item()) == 0


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_two_runs_give_the_same_bits(precision):
    hw, depth, B, K, _, _ = R.CASES["k64"]
    p, img, idx, r, rl = R.case_inputs("k64")
    m = build(p, hw, depth, precision)

    def go():
        for prm in m.parameters():
            prm.grad = None
        x = img.to(DEV).requires_grad_(True)
        f = m.features3D(x, keep_indices=idx.to(DEV))
        (f * r.to(DEV)).sum().backward()
        return [f.detach().clone(), x.grad.clone()] + [prm.grad.clone() for prm in m.parameters() if prm.grad is not None]
    a, b = go(), go()
    assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("bucket", [1, 2])
def test_staged_backward_matches_the_single_call(bucket):
    depth = 3
    p = R.params_for(9301, (64, 64), depth)
    m = build(p, (64, 64), depth, "fp32")
    x = R.rng(9302, (2, 3, 64, 64)).to(DEV).requires_grad_(True)
    idx = R.rng_indices(9303, 2, 16, 7).to(DEV)
    w = R.rng(9304, (2, 8, 384)).to(DEV)

    def grads():
        for prm in m.parameters():
            prm.grad = None
        x.grad = None
        (m.features3D(x, keep_indices=idx) * w).sum().backward()
        out = {k: prm.grad.detach().clone() for k, prm in m.named_parameters() if prm.grad is not None}
        out["d img"] = x.grad.clone()
        return out
    ref = grads()
    seen = []
    m._grad_bucket_layers = bucket
    m._grad_stage_hook = lambda vit, hi, lo, gflat: seen.append((hi, lo))
    got = grads()
    del m._grad_stage_hook
    assert [s for hi, lo in seen for s in range(hi, lo - 1, -1)] == list(range(depth, -2, -1)), seen
    assert set(got) == set(ref)
    for k in ref:
        assert R.scale_err(got[k], ref[k]) < 1e-5, k


def test_drop_path_combined_with_patch_dropout():
    """The fine-tune recipe: drop_path_rate and patch dropout together, against the restatement fed with the kernels' own per-sample keep
    factors (mfvit_dropout_mask, as tests/test_vit_dropout_gpu.py obtains them)."""
    from mfvit import ops
    hw, depth, B, K = (64, 64), 3, 3, 9
    p = R.params_for(9401, hw, depth)
    m = build(p, hw, depth, "bf16x3", drop_path_rate=0.5)
    img, idx = R.rng(9402, (B, 3) + hw), R.rng_indices(9403, B, 16, K)
    r = R.rng(9404, (B, 1 + K, 384))
    torch.manual_seed(3)
    x = img.to(DEV).requires_grad_(True)
    f = m.features3D(x, keep_indices=idx.to(DEV))
    (f * r.to(DEV)).sum().backward()
    _, _, dpr = m.drop_rates()
    seed = m._last_drop.seed
    fac = torch.ones(depth, 2, B, dtype=torch.float64)
    for l in range(depth):
        if dpr[l] > 0:
            for j, site in enumerate((16 * l + 6, 16 * l + 7)):
                fac[l, j] = ops.dropout_mask(dpr[l], seed, site, B).double().cpu() / (1.0 - dpr[l])
    assert 0 < int((fac == 0).sum()) < fac.numel() - 2 * B, "the seed must drop some, not all, of the branches"
    ref = R.run(p, img, idx, r, torch.zeros(B, 3), torch.float64, path_factors=fac)
    e_f = R.scale_err(f, ref["features"])
    e_g = max(R.scale_err(prm.grad, ref["grads"][k]) for k, prm in m.named_parameters() if prm.grad is not None)
    e_d = R.scale_err(x.grad, ref["dimg"])
    log(f"drop path + patch dropout [bf16x3] features {e_f:.2e} grads {e_g:.2e} dimg {e_d:.2e}")
    cap_f, cap_g = R.CAPS["bf16x3"]
    assert e_f < cap_f and e_g < cap_g and e_d < cap_g, (e_f, e_g, e_d)


# --------------------------------------------------------------------------------------------------- the random draw
def test_random_draw_shape_range_and_reproducibility():
    hw, depth, B = (64, 64), 2, 3
    p = R.params_for(9501, hw, depth)
    m = build(p, hw, depth, "bf16x3", patch_drop_rate=0.5)
    x = R.rng(9502, (B, 3) + hw).to(DEV)

    def step():
        f = m.features3D(x)
        return f.detach().clone(), m.last_keep_indices.clone()
    torch.manual_seed(11)
    f1, i1 = step()
    f2, i2 = step()
    assert f1.shape == (B, 1 + 8, 384) and i1.shape == (B, 8) and i1.dtype == torch.int64
    for i in (i1, i2):
        assert int(i.min()) >= 0 and int(i.max()) < 16
        assert all(len(set(row)) == 8 for row in i.cpu().tolist())
    assert not torch.equal(i1, i2), "two steps must draw different patches"
    torch.manual_seed(11)
    g1, j1 = step()
    g2, j2 = step()
    assert torch.equal(i1, j1) and torch.equal(i2, j2) and torch.equal(f1, g1) and torch.equal(f2, g2)
    mo = build(p, hw, depth, "bf16x3", patch_drop_rate=0.5, patch_drop_ordered=True)
    mo.features3D(x)
    io = mo.last_keep_indices
    assert torch.equal(io, io.sort(dim=-1)[0])
    m.eval()
    with torch.no_grad():
        assert m.features3D(x).shape == (B, 17, 384)


# --------------------------------------------------------------------------------------------------- refusals: none reaches a kernel
def test_refusals_launch_nothing():
    from mfvit import lora
    hw, depth, B = (64, 64), 2, 2
    p = R.params_for(9601, hw, depth)
    m = build(p, hw, depth, "bf16x3", patch_drop_rate=0.5)
    x = R.rng(9602, (B, 3) + hw).to(DEV)
    calls = []
    real = m._forward_chain                         # (img, idx, plan, ..): every encoder forward; 1: on kept-patch indices, 0: without
    m._forward_chain = lambda *a, **k: calls.append(int(a[1] is not None)) or real(*a, **k)
    good = torch.tensor([[0, 5, 3], [15, 2, 7]], device=DEV)
    for bad in (torch.tensor([[0, 5, 16], [1, 2, 3]], device=DEV), torch.tensor([[0, 5, -1], [1, 2, 3]], device=DEV),
                torch.tensor([[0, 5, 5], [1, 2, 3]], device=DEV), torch.tensor([[0, 5, 3]], device=DEV),
                torch.tensor([[0.0, 5.0, 3.0], [1.0, 2.0, 3.0]], device=DEV), torch.zeros(B, 0, dtype=torch.long, device=DEV)):
        with pytest.raises(MfvitError):
            m.features3D(x, keep_indices=bad)
    m.eval()
    with pytest.raises(MfvitError):
        m.features3D(x, keep_indices=good)
    with pytest.raises(MfvitError):
        m(x, keep_indices=good)
    m.train()
    lora.add_lora(m, rank=4)
    with pytest.raises(MfvitError, match="LoRA"):
        m.features3D(x)
    with pytest.raises(MfvitError, match="LoRA"):
        m.features3D(x, keep_indices=good)
    assert calls == []
    lora.remove_lora(m)
    assert m.features3D(x, keep_indices=good).shape == (B, 4, 384) and calls == [1]
    m.check_keep_error()


# --------------------------------------------------------------------------------------------------- evaluation paths are untouched
def test_evaluation_paths_equal_the_model_without_patch_dropout():
    hw, depth, B = (64, 64), 2, 2
    p = R.params_for(9701, hw, depth)
    x = R.rng(9702, (B, 3) + hw).to(DEV)
    m0, m1 = build(p, hw, depth, "bf16x3"), build(p, hw, depth, "bf16x3", patch_drop_rate=0.5)      # (both in training mode)
    for a, b in zip(m0.get_attention_maps(x), m1.get_attention_maps(x)):
        assert torch.equal(a, b)
    assert torch.equal(m0.attention_relevance(x, target=1), m1.attention_relevance(x, target=1))
    assert torch.equal(m0.hidden_states(x), m1.hidden_states(x))
    s0, s1 = m0.attention_stats(x), m1.attention_stats(x)
    assert set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert torch.equal(m0.attention_rollout(x), m1.attention_rollout(x))
    m0.eval(), m1.eval()
    with torch.no_grad():
        assert torch.equal(m0.features3D(x), m1.features3D(x)) and torch.equal(m0(x), m1(x))


# --------------------------------------------------------------------------------------------------- Fus_CrossViT
def build_fus(rate, shared, depth=2, hw=(64, 64), precision="bf16x3"):
    fus = importlib.import_module(FUS_MOD)
    ps = [R.params_for(9801 + i, hw, depth) for i in range(2)]
    backs = [build(q, hw, depth, precision, patch_drop_rate=rate) for q in ps]
    model = fus.Fus_CrossViT(backs[0], backs[1], patch_drop_shared=shared)
    fp = ref_fusion.seeded_fusion_params(9803)
    model.load_state_dict(fp)
    return model.to(DEV).train(), backs, fp


def count_backbone_forwards(vit, calls):
    real = vit._forward_chain                       # (img, idx, plan, ..): "keep" when the call was given kept-patch indices
    vit._forward_chain = lambda *a, **k: calls.append("full" if a[1] is None else "keep") or real(*a, **k)


@pytest.mark.parametrize("shared", [True, False])
def test_fus_crossvit_train_step_on_the_kept_tokens(shared):
    B, K = 3, 8
    model, (vc, ve), fp = build_fus(0.5, shared)
    calls_c, calls_e = [], []
    count_backbone_forwards(vc, calls_c)
    count_backbone_forwards(ve, calls_e)
    x, xe = R.rng(9811, (B, 3, 64, 64)).to(DEV), R.rng(9812, (B, 3, 64, 64)).to(DEV)
    torch.manual_seed(5)
    fused, x_c, x_e = model(vc, ve, x, xe)
    assert calls_c == ["keep"] and calls_e == ["keep"], (calls_c, calls_e)      # one backbone forward per encoder per step
    ic, ie = vc.last_keep_indices, ve.last_keep_indices
    assert ic.shape == (B, K) and ie.shape == (B, K)
    assert torch.equal(ic, ie) == shared
    (fused + x_c + x_e).sum().backward()
    for vit in (vc, ve):      # gradients reach both encoders' arenas
        assert all(prm.grad is not None and torch.isfinite(prm.grad).all() and float(prm.grad.abs().max()) > 0
                   for k, prm in vit.named_parameters() if k != "pos_embed" and not k.startswith("head")), "encoder gradients"
        assert vit.blocks[0].attn.qkv.weight.grad.data_ptr() == vit._last_grad_arena.data_ptr() + 4 * vit.arena_slice("blocks.0.attn.qkv.weight")[0]
    # the encoders' own dropped features (explicit indices: the same bits, test_two_runs_give_the_same_bits) through the float64 fusion oracle
    with torch.no_grad():
        fc, fe_ = vc.features3D(x, keep_indices=ic), ve.features3D(xe, keep_indices=ie)
    assert fc.shape == (B, 1 + K, 384) and fe_.shape == (B, 1 + K, 384)
    pd = {k: v.double() for k, v in fp.items()}
    r_fused, r_c, r_e = ref_fusion.fus_ex_forward(pd, fc.double().cpu(), fe_.double().cpu(), hw_cxr=vc.head.weight.detach().double().cpu(),
                                                  hb_cxr=vc.head.bias.detach().double().cpu(), hw_enh=ve.head.weight.detach().double().cpu(),
                                                  hb_enh=ve.head.bias.detach().double().cpu())
    errs = [R.scale_err(a, b) for a, b in ((fused, r_fused), (x_c, r_c), (x_e, r_e))]
    log(f"Fus_CrossViT on kept tokens [shared={shared}] fused / x_cxr / x_enh {errs}")
    assert max(errs) < FUSION_GATES["out"], errs
    vc.check_keep_error(), ve.check_keep_error()


def test_fus_crossvit_eval_equals_the_model_without_patch_dropout():
    B = 2
    x, xe = R.rng(9821, (B, 3, 64, 64)).to(DEV), R.rng(9822, (B, 3, 64, 64)).to(DEV)
    outs = []
    for rate in (0.0, 0.5):
        model, (vc, ve), _ = build_fus(rate, True)
        model.eval(), vc.eval(), ve.eval()
        with torch.no_grad():
            outs.append(model(vc, ve, x, xe))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
