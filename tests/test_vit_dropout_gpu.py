"""Training-mode dropout / attention dropout / stochastic depth of the ViT encoder (timm 0.4.9 semantics, include/mfvit.h mfvit_vit_drop).

torch's mask stream cannot be reproduced, so every parity test exports the keep masks the kernels drew for the forward under test
(mfvit_dropout_mask: same (p, seed, site) -> same bits) and runs a float64 reference built from oracle.ref_vit primitives with exactly
those masks."""
import importlib

import pytest
import torch

from conftest import rng_tensor
from oracle import ref_fusion, ref_vit

DEV = "cuda:0"
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
TOL = {"bf16x3": 1e-3, "fp16": 1e-2, "bf16": 4e-2}


def rel_err(got, ref):
    ref, got = ref.detach().double().cpu(), got.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def build(arch, depth, precision, seed=7, **rates):
    import vits
    m = getattr(vits, arch)(num_classes=3, depth=depth, precision=precision, **rates)
    sd = ref_vit.seeded_params(seed, arch=arch, num_classes=3, depth=depth)
    m.load_state_dict(sd)
    return m.to(DEV).train(), sd


def masks_of(model, B, T, heads):
    """The keep masks (float 0 / 1) of the model's last training-mode forward, per timm site."""
    from mfvit import ops
    d = model._last_drop
    drop, attn, dpr = model.drop_rates()
    D, F = model.embed_dim, model.mlp_dim
    mk = {}

    def get(p, site, n, shape):
        return ops.dropout_mask(p, d.seed, site, n).reshape(shape).double().cpu()
    if drop > 0:
        mk["pos"] = get(drop, 1, B * T * D, (B, T, D))
    for l in range(model.depth):
        if attn > 0:
            mk["attn", l] = get(attn, 16 * l + 2, B * heads * T * T, (B, heads, T, T))
        if drop > 0:
            mk["proj", l] = get(drop, 16 * l + 3, B * T * D, (B, T, D))
            mk["fc2", l] = get(drop, 16 * l + 4, B * T * D, (B, T, D))
            mk["gelu", l] = get(drop, 16 * l + 5, B * T * F, (B, T, F))
        if dpr[l] > 0:
            mk["dp_attn", l] = get(dpr[l], 16 * l + 6, B, (B, 1, 1))
            mk["dp_mlp", l] = get(dpr[l], 16 * l + 7, B, (B, 1, 1))
    return mk, (drop, attn, dpr)


def ref_logits(p, img, heads, mk, rates):
    """timm VisionTransformer.forward in float64 with the given keep masks (training mode)."""
    drop, attn, dpr = rates
    LN = ref_vit.LN_EPS

    def dr(x, key, rate):
        return x * mk[key] / (1.0 - rate) if key in mk else x
    B = img.shape[0]
    x = ref_vit.patch_embed(p, img)
    x = torch.cat([p["cls_token"].expand(B, -1, -1), x], dim=1) + p["pos_embed"]
    x = dr(x, "pos", drop)
    for i in range(ref_vit.depth_of(p)):
        pre = f"blocks.{i}."
        y = ref_vit.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], LN)
        Bq, T, D = y.shape
        hd = D // heads
        qkv = (y @ p[pre + "attn.qkv.weight"].t() + p[pre + "attn.qkv.bias"]).reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = ((qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
        a = dr(a, ("attn", i), attn)
        o = (a @ qkv[2]).transpose(1, 2).reshape(B, T, D) @ p[pre + "attn.proj.weight"].t() + p[pre + "attn.proj.bias"]
        x = x + dr(dr(o, ("proj", i), drop), ("dp_attn", i), dpr[i])
        y = ref_vit.layer_norm(x, p[pre + "norm2.weight"], p[pre + "norm2.bias"], LN)
        h = dr(ref_vit.gelu_erf(y @ p[pre + "mlp.fc1.weight"].t() + p[pre + "mlp.fc1.bias"]), ("gelu", i), drop)
        o = h @ p[pre + "mlp.fc2.weight"].t() + p[pre + "mlp.fc2.bias"]
        x = x + dr(dr(o, ("fc2", i), drop), ("dp_mlp", i), dpr[i])
    f = ref_vit.layer_norm(x, p["norm.weight"], p["norm.bias"], LN)
    return f[:, 0] @ p["head.weight"].t() + p["head.bias"]


SITES = {
    "pos+proj+mlp": dict(drop_rate=0.2),
    "attn": dict(attn_drop_rate=0.2),
    "drop_path": dict(drop_path_rate=0.5),
    "all": dict(drop_rate=0.1, attn_drop_rate=0.15, drop_path_rate=0.4),
}


def run_parity(arch, depth, B, precision, rates, grads, seed=11):
    heads = 12
    m, sd = build(arch, depth, precision, **rates)
    img = rng_tensor(41 + B, (B, 3, 224, 224))
    torch.manual_seed(seed)
    logits = m(img.to(DEV))
    T = m.num_tokens
    mk, rr = masks_of(m, B, T, heads)
    w = rng_tensor(43, (B, 3)).to(DEV)
    if grads:
        (logits * w).sum().backward()
    pd = {k: v.double().requires_grad_(k != "pos_embed") for k, v in sd.items()}
    r = ref_logits(pd, img.double(), heads, mk, rr)
    out = {"logits": rel_err(logits, r)}
    if grads:
        (r * w.double().cpu()).sum().backward()
        named = dict(m.named_parameters())
        gmax = max(float(v.grad.abs().max()) for v in pd.values() if v.grad is not None)
        worst = ("", 0.0)
        for k, v in pd.items():
            if v.grad is None or float(v.grad.abs().max()) < 1e-3 * gmax:
                continue
            e = rel_err(named[k].grad, v.grad)
            if e > worst[1]:
                worst = (k, e)
        out["grad"] = worst
    return out, mk


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16"])
@pytest.mark.parametrize("sites", list(SITES))
@pytest.mark.parametrize("arch,depth,B", [("vit_small", 3, 3), ("vit_base", 2, 2)])
def test_forward_matches_reference_with_the_same_masks(arch, depth, B, precision, sites):
    """Each site alone, then all together; B * 197 rows are not a multiple of any tile height."""
    out, mk = run_parity(arch, depth, B, precision, SITES[sites], grads=False)
    assert mk, "no masks drawn: the rates did not reach the kernels"
    assert out["logits"] < TOL[precision], out


@pytest.mark.gpu
@pytest.mark.parametrize("sites", list(SITES))
@pytest.mark.parametrize("arch,depth,B", [("vit_small", 4, 3), ("vit_base", 2, 2)])
def test_backward_matches_reference_at_the_bf16x3_gate(arch, depth, B, sites):
    out, _ = run_parity(arch, depth, B, "bf16x3", SITES[sites], grads=True)
    assert out["logits"] < 1e-3 and out["grad"][1] < 1e-3, out


def _seed_dropping_a_whole_sample(depth, rate, B):
    """A torch seed whose drawn mask seed drops BOTH branches of every block with rate > 0 for some sample."""
    from mfvit import ops
    dpr = [x.item() for x in torch.linspace(0, rate, depth)]
    for k in range(500):
        torch.manual_seed(k)
        s = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        dropped_all = torch.ones(B, dtype=torch.bool)
        for l in range(1, depth):
            for site in (16 * l + 6, 16 * l + 7):
                dropped_all &= ~ops.dropout_mask(dpr[l], s, site, B).cpu()
        if bool(dropped_all.any()) and not bool(dropped_all.all()):
            return k
    raise AssertionError("no seed found")


@pytest.mark.gpu
def test_backward_with_a_sample_whose_every_branch_is_dropped():
    depth, B = 3, 4
    k = _seed_dropping_a_whole_sample(depth, 0.8, B)
    out, mk = run_parity("vit_small", depth, B, "bf16x3", dict(drop_path_rate=0.8), grads=True, seed=k)
    gone = torch.ones(B, dtype=torch.bool)
    for l in (1, 2):
        gone &= (mk["dp_attn", l].flatten() == 0) & (mk["dp_mlp", l].flatten() == 0)
    assert bool(gone.any())
    assert out["logits"] < 1e-3 and out["grad"][1] < 1e-3, out


def _step(m, img, y):
    from mfvit.losses import cross_entropy
    for p in m.parameters():
        p.grad = None
    logits = m(img)
    loss, _ = cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return [logits.detach().clone(), loss.detach().clone()] + [p.grad.detach().clone() for p in m.parameters() if p.grad is not None]


@pytest.mark.gpu
def test_train_and_eval_behaviour():
    img = rng_tensor(51, (2, 3, 224, 224)).to(DEV)
    y = torch.tensor([0, 2], device=DEV)
    m, _ = build("vit_small", 3, "bf16x3", drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2)
    with torch.no_grad():
        a, b = m(img), m(img)
    assert not torch.equal(a, b), "two training-mode forwards gave the same logits"
    z, _ = build("vit_small", 3, "bf16x3")
    m.eval()
    z.eval()
    with torch.no_grad():
        assert torch.equal(m(img), z(img))                    # eval(): today's kernels, today's bits
    # rates 0 in training mode run the encoder without a mfvit_vit_drop, exactly like a model built without the kwargs: logits and every gradient
    # bit for bit.  (Both sides run this change's code; that the rates-0 bits equal the previous sources' is shown by `bench.py --dump-outputs`
    # before / after, profiles/README.md.)
    r0, _ = build("vit_small", 3, "bf16x3", drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)
    z.train()
    for u, v in zip(_step(r0, img, y), _step(z, img, y)):
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_training_step_is_reproducible_under_manual_seed():
    img = rng_tensor(52, (3, 3, 224, 224)).to(DEV)
    y = torch.tensor([0, 2, 1], device=DEV)
    m, _ = build("vit_small", 3, "bf16x3", drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2)
    torch.manual_seed(3)
    r1 = _step(m, img, y)
    torch.manual_seed(3)
    r2 = _step(m, img, y)
    assert len(r1) > 10
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    torch.manual_seed(4)
    assert not torch.equal(_step(m, img, y)[0], r1[0])


def _ca_model(rates, depth=2):
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    backs = []
    for i in range(2):
        m = vits.vit_small(num_classes=3, depth=depth, **rates)
        m.load_state_dict(ref_vit.seeded_params(7 + i, num_classes=3, depth=depth))
        backs.append(m.to(DEV).train())
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(ref_fusion.seeded_fusion_params(9))
    return model.to(DEV).train(), backs


def _ca_step(model, backs, x, xe, y):
    from mfvit.losses import cross_entropy
    for mod in [model] + backs:
        for p in mod.parameters():
            p.grad = None
    fused, x_c, x_e = model(backs[0], backs[1], x, xe)
    loss, _ = cross_entropy(fused + x_c + x_e, y)
    loss.backward()
    torch.cuda.synchronize()
    out = [fused.detach().clone(), x_c.detach().clone(), x_e.detach().clone(), loss.detach().clone()]
    for mod in [model] + backs:
        out += [p.grad.detach().clone() for p in mod.parameters() if p.grad is not None]
    return out


@pytest.mark.gpu
def test_two_stream_ca_step_is_reproducible_and_heads_use_forwards_of_their_own():
    rates = dict(drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2)
    model, backs = _ca_model(rates)
    x, xe = rng_tensor(61, (2, 3, 224, 224)).to(DEV), rng_tensor(62, (2, 3, 224, 224)).to(DEV)
    y = torch.tensor([1, 2], device=DEV)
    seeds, forwards = [], []
    for b in backs:
        orig, orig_fwd = b._draw_drop, b._forward_chain

        def rec(orig=orig):
            d = orig()
            if d is not None:
                seeds.append(d.seed)
            return d

        def rec_fwd(*a, orig_fwd=orig_fwd, **k):
            assert a[1] is None and len(a[2]) == 1      # (img, idx, plan, ..): the full grid - no kept-patch indices, one block range
            forwards.append(1)
            return orig_fwd(*a, **k)
        b._draw_drop = rec
        b._forward_chain = rec_fwd
    torch.manual_seed(9)
    r1 = _ca_step(model, backs, x, xe, y)
    # x_cxr / x_enh come from forwards independent of the fused features: 2 backbones x (features3D + __call__) = 4 mask seeds
    assert len(seeds) == 4 and len(set(seeds)) == 4, seeds
    assert len(forwards) == 4
    torch.manual_seed(9)
    r2 = _ca_step(model, backs, x, xe, y)
    assert len(r1) == len(r2) > 20
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    assert seeds[:4] == seeds[4:8]
    # without dropout (eval) the fused-heads shortcut is back: ONE encoder forward per backbone, no masks
    for b in backs:
        b.eval()
    seeds.clear()
    forwards.clear()
    with torch.no_grad():
        model(backs[0], backs[1], x, xe)
    assert seeds == [] and len(forwards) == 2


def _prof_counts(fn):
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


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16"])
def test_drop_path_only_forward_stays_on_the_row_complete_kernels(precision):
    """The fine-tune recipe (drop_rate = attn_drop_rate = 0, drop_path_rate > 0) on vit_small: the forward launches exactly the kernel classes of
    a rates-0 forward - both residual adds of every block on the row-complete GEMM (class 1, gemm_nt_row_res_ln), no tile GEMM + row pass in
    their place - while drop_rate > 0 moves them off it (the observable can tell the two apart)."""
    depth, B = 4, 12                                    # 2,364 token rows: the bench-like regime of the persistent tile kernel too
    img = rng_tensor(71, (B, 3, 224, 224)).to(DEV)
    z, _ = build("vit_small", depth, precision)
    dp, _ = build("vit_small", depth, precision, drop_path_rate=0.3)
    dr, _ = build("vit_small", depth, precision, drop_rate=0.1)

    def fwd(m):
        def run():
            with torch.no_grad():
                m.features3D(img)
        return run
    cz, cdp, cdr = _prof_counts(fwd(z)), _prof_counts(fwd(dp)), _prof_counts(fwd(dr))
    assert dp._last_drop is not None and cz[1] == 2 * depth + 1, (cz, cdp)       # + 1: the patch embedding
    assert cdp[0] == cz[0] and cdp[1] == cz[1], (cz, cdp)
    assert cdr[1] == 1 and cdr[0] > cz[0], (cz, cdr)


@pytest.mark.gpu
def test_gelu_dropout_on_the_persistent_tile_kernel(monkeypatch):
    """fc1 + GELU-site dropout on the persistent ping-pong kernel (gemm_pp.hip), which takes fc1 at >= 2,048 token rows - every training batch:
    MFVIT_PP=2 puts it wherever it can run, so a B = 3 forward / backward exercises its EPI_BIAS_GELU_DROP epilogue against the reference."""
    monkeypatch.setenv("MFVIT_PP", "2")
    out, mk = run_parity("vit_small", 2, 3, "bf16x3", dict(drop_rate=0.2), grads=True)
    assert ("gelu", 0) in mk
    assert out["logits"] < 1e-3 and out["grad"][1] < 1e-3, out


@pytest.mark.gpu
def test_gelu_dropout_at_a_training_batch():
    """The same at B = 12 (2,364 token rows) with the library's default kernel choice."""
    out, mk = run_parity("vit_small", 2, 12, "bf16x3", dict(drop_rate=0.1, drop_path_rate=0.2), grads=True)
    assert out["logits"] < 1e-3 and out["grad"][1] < 1e-3, out
