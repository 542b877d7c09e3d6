"""LoRA adapters, the parts that need no GPU: the algebra the kernels and the references rest on, the gates' power to catch wrong kernels, and
the host surface of mfvit.lora on a CPU-constructed model (names, shapes, init, freezing, state dicts, merge / remove, every refusal)."""
import math

import pytest
import torch
import torch.nn.functional as F

import lora_ref


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ algebra
def test_merged_linear_equals_the_unmerged_form_in_float64():
    g = gen(1)
    N, K, r, s = 24, 40, 5, 2.0
    x = torch.randn(7, K, generator=g, dtype=torch.float64)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    A = torch.randn(r, K, generator=g, dtype=torch.float64)
    B = torch.randn(N, r, generator=g, dtype=torch.float64)
    merged = F.linear(x, W + s * B @ A)
    unmerged = F.linear(x, W) + s * F.linear(F.linear(x, A), B)
    assert float((merged - unmerged).abs().max()) <= 1e-12 * float(merged.abs().max())


def test_chain_rule_through_the_merged_weight_matches_autograd():
    g = gen(2)
    N, K, r, s = 12, 16, 3, 0.75
    x = torch.randn(9, K, generator=g, dtype=torch.float64)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    A = torch.randn(r, K, generator=g, dtype=torch.float64, requires_grad=True)
    B = torch.randn(N, r, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(9, N, generator=g, dtype=torch.float64)
    (F.linear(x, W + s * B @ A) * dy).sum().backward()
    dW = dy.t() @ x
    assert torch.allclose(A.grad, s * B.detach().t() @ dW, rtol=1e-12, atol=1e-12)
    assert torch.allclose(B.grad, s * dW @ A.detach().t(), rtol=1e-12, atol=1e-12)


def test_merged_dict_puts_q_k_v_on_their_own_row_blocks():
    from oracle import ref_vit
    sd = ref_vit.seeded_params(3, num_classes=3, depth=1)
    s = 2.0
    ad = lora_ref.seeded_adapters(4, sd, 4, [0], ("q", "k", "v", "fc2"), s)
    pd = {k: v.double() for k, v in sd.items()}
    m = lora_ref.merged(pd, ad, s, [0], ("q", "k", "v", "fc2"))
    D = 384
    for rb, t in enumerate("qkv"):
        upd = s * ad[f"blocks.0.attn.qkv.lora_B_{t}"].double() @ ad[f"blocks.0.attn.qkv.lora_A_{t}"].double()
        got = (m["blocks.0.attn.qkv.weight"] - pd["blocks.0.attn.qkv.weight"])[rb * D:(rb + 1) * D]
        assert torch.allclose(got, upd, rtol=0, atol=1e-15)
    assert ad["blocks.0.mlp.fc2.lora_A"].shape == (4, 1536) and ad["blocks.0.mlp.fc2.lora_B"].shape == (384, 4)
    assert torch.equal(m["blocks.0.attn.proj.weight"], pd["blocks.0.attn.proj.weight"])
    # the B's are scaled to the stated size of the update
    w = pd["blocks.0.mlp.fc2.weight"]
    upd = m["blocks.0.mlp.fc2.weight"] - w
    assert abs(float(upd.abs().max()) / float(w.abs().max()) - 2.0 ** -6) < 1e-6 * 2.0 ** -6


def test_split_bf16_grid_keeps_sixteen_bits():
    x = torch.randn(4096, generator=gen(5), dtype=torch.float64)
    e = ((lora_ref.round_split_bf16(x) - x).abs() / x.abs()).max()
    assert 2.0 ** -19 < float(e) <= 2.0 ** -16          # hi + lo: 8 + 8 mantissa bits and the sign trick, never worse than 2^-16


# ------------------------------------------------------------------------------------------------ the gates catch wrong kernels
def _f32_kernel_model(w, a, b, s):
    """What a correct f32 kernel may return: the float64 result rounded once to f32 (inside every gate by construction)."""
    return (w.double() + s * (b.double() @ a.double())).float()


@pytest.mark.parametrize("mutation", ["no_scale", "transpose_a", "k_on_q_rows"])
def test_each_gate_catches_the_mutation(mutation):
    g = gen(6)
    N = K = r = 8                                        # square everywhere: A^T has A's shape, and a row block has the adapter's height
    s = 0.25
    W = torch.randn(3 * N, K, generator=g)               # a fused q | k | v matrix
    A = torch.randn(r, K, generator=g)
    Bk = torch.randn(N, r, generator=g)
    dW = torch.randn(3 * N, K, generator=g)
    rows_k, rows_q = slice(N, 2 * N), slice(0, N)
    # the correct results for the k block pass all three gates
    ref, gate = lora_ref.merge_ref_and_gate(W[rows_k], A, Bk, s)
    assert lora_ref.within(_f32_kernel_model(W[rows_k], A, Bk, s), ref, gate) <= 1.0
    (da, ga), (db, gb) = lora_ref.grad_ref_and_gate(dW[rows_k], A, Bk, s)
    assert lora_ref.within(da.float(), da, ga) <= 1.0 and lora_ref.within(db.float(), db, gb) <= 1.0
    # the mutants
    s_m = 1.0 if mutation == "no_scale" else s
    A_m = A.t().contiguous() if mutation == "transpose_a" else A
    rows_m = rows_q if mutation == "k_on_q_rows" else rows_k
    merged_m = W.clone().double()
    merged_m[rows_m] += s_m * (Bk.double() @ A_m.double())
    full_ref = W.clone().double()
    full_ref[rows_k] = ref
    full_gate = 3 * lora_ref.U * W.double().abs()        # rows without an update: w itself (any positive gate would do)
    full_gate[rows_k] = gate
    assert lora_ref.within(merged_m.float(), full_ref, full_gate) > 1.0
    da_m = s_m * (Bk.double().t() @ dW[rows_m].double()) if mutation != "transpose_a" else s * (Bk.double().t() @ dW[rows_k].double()).t()
    db_m = s_m * (dW[rows_m].double() @ A_m.double().t())
    assert lora_ref.within(da_m.float(), da, ga) > 1.0
    assert lora_ref.within(db_m.float(), db, gb) > 1.0


# ------------------------------------------------------------------------------------------------ host surface
def small(depth=2, precision="bf16x3", arch="vit_small"):
    import vits
    return getattr(vits, arch)(num_classes=3, depth=depth, precision=precision)


def test_default_adapters_names_shapes_init_and_count():
    from mfvit import lora
    m = small(depth=12)
    keys_before = set(m.state_dict().keys())
    ps = lora.add_lora(m, generator=gen(7))
    assert len(ps) == 12 * 2 * 2 and all(p.is_leaf and p.dtype == torch.float32 for p in ps)
    named = dict(m.named_parameters())
    for i in range(12):
        for t in "qv":
            a, b = named[f"blocks.{i}.attn.qkv.lora_A_{t}"], named[f"blocks.{i}.attn.qkv.lora_B_{t}"]
            assert a.shape == (8, 384) and b.shape == (384, 8)
            assert float(b.detach().abs().max()) == 0.0
            assert 0.5 / math.sqrt(384) < float(a.detach().abs().max()) <= 1 / math.sqrt(384)
        assert f"blocks.{i}.attn.qkv.lora_A_k" not in named
    trainable = sum(p.numel() for n, p in m.named_parameters() if p.requires_grad and not n.startswith("head."))
    assert trainable == 12 * 2 * (8 * 384 + 384 * 8) == 147456
    assert all(not p.requires_grad for _, p in m.arena_named_parameters())
    assert m.head.weight.requires_grad and m.head.bias.requires_grad
    assert set(m.state_dict().keys()) - keys_before == {k for k in named if "lora_" in k}
    assert [id(p) for p in lora.lora_parameters(m)] == [id(p) for p in ps]
    # same generator seed, same A
    m2 = small(depth=12)
    ps2 = lora.add_lora(m2, generator=gen(7))
    assert all(torch.equal(p, q) for p, q in zip(ps, ps2))


def test_all_targets_selected_blocks_and_rslora():
    from mfvit import lora
    m = small(depth=4)
    lora.add_lora(m, rank=4, alpha=8.0, targets=("fc2", "q", "k", "v", "proj", "fc1"), blocks=[-1, 1], rslora=True, freeze_base=False)
    named = dict(m.named_parameters())
    assert m._lora.scale == 8.0 / 2.0
    for i in (1, 3):
        assert named[f"blocks.{i}.attn.proj.lora_A"].shape == (4, 384) and named[f"blocks.{i}.attn.proj.lora_B"].shape == (384, 4)
        assert named[f"blocks.{i}.mlp.fc1.lora_A"].shape == (4, 384) and named[f"blocks.{i}.mlp.fc1.lora_B"].shape == (1536, 4)
        assert named[f"blocks.{i}.mlp.fc2.lora_A"].shape == (4, 1536) and named[f"blocks.{i}.mlp.fc2.lora_B"].shape == (384, 4)
        assert float(named[f"blocks.{i}.mlp.fc2.lora_A"].detach().abs().max()) <= 1 / math.sqrt(1536)
        for t in "qkv":
            assert f"blocks.{i}.attn.qkv.lora_A_{t}" in named
    assert not any("lora_" in k and (k.startswith("blocks.0.") or k.startswith("blocks.2.")) for k in named)
    assert m.blocks[0].attn.qkv.weight.requires_grad                     # freeze_base=False leaves the flags alone
    b = small(depth=2, arch="vit_base")
    lora.add_lora(b, rank=64, targets=("fc1",))
    assert dict(b.named_parameters())["blocks.0.mlp.fc1.lora_B"].shape == (3072, 64)


def test_state_dict_round_trip_merge_and_remove_restore_the_key_set():
    from mfvit import lora
    m = small()
    keys = set(m.state_dict().keys())
    flags = {n: p.requires_grad for n, p in m.named_parameters()}
    base = {k: v.clone() for k, v in m.state_dict().items()}
    lora.add_lora(m, rank=2, targets=("q", "fc1"), generator=gen(8))
    with torch.no_grad():
        for p in lora.lora_parameters(m):
            p.copy_(torch.randn(p.shape, generator=gen(9)))
    sd = lora.lora_state_dict(m)
    assert set(sd) == {k for k in m.state_dict() if "lora_" in k} and len(sd) == 2 * 2 * 2
    m2 = small()
    lora.add_lora(m2, rank=2, targets=("q", "fc1"))
    assert lora.load_lora_state_dict(m2, sd) == ([], [])
    assert all(torch.equal(sd[k], v) for k, v in lora.lora_state_dict(m2).items())
    with pytest.raises(RuntimeError, match="unexpected"):
        lora.load_lora_state_dict(m2, dict(sd, extra=torch.zeros(1)))
    part = dict(list(sd.items())[:2])
    with pytest.raises(RuntimeError, match="missing"):
        lora.load_lora_state_dict(m2, part)
    missing, unexpected = lora.load_lora_state_dict(m2, part, strict=False)
    assert len(missing) == len(sd) - 2 and unexpected == []
    with pytest.raises(RuntimeError, match="shape"):
        lora.load_lora_state_dict(m2, {k: v[:1] for k, v in sd.items()})
    # remove: the base bits, keys and flags come back
    lora.remove_lora(m2)
    assert set(m2.state_dict().keys()) == keys and not lora.has_lora(m2)
    assert {n: p.requires_grad for n, p in m2.named_parameters()} == flags
    # merge: keys and flags come back, the adapted weights moved by s B A, everything else kept its bits
    s = m._lora.scale
    upd = s * sd["blocks.1.mlp.fc1.lora_B"].double() @ sd["blocks.1.mlp.fc1.lora_A"].double()
    lora.merge_lora(m)
    after = m.state_dict()
    assert set(after.keys()) == keys and {n: p.requires_grad for n, p in m.named_parameters()} == flags
    got = after["blocks.1.mlp.fc1.weight"].double() - base["blocks.1.mlp.fc1.weight"].double()
    assert float((got - upd).abs().max()) <= 4 * lora_ref.U * float((base["blocks.1.mlp.fc1.weight"].abs().max() + upd.abs().max()))
    D = 384
    assert not torch.equal(after["blocks.0.attn.qkv.weight"][:D], base["blocks.0.attn.qkv.weight"][:D])
    assert torch.equal(after["blocks.0.attn.qkv.weight"][D:], base["blocks.0.attn.qkv.weight"][D:])
    assert torch.equal(after["blocks.0.attn.proj.weight"], base["blocks.0.attn.proj.weight"])
    assert m._arena_intact()
    lora.add_lora(m)                                                      # and adapters can be attached again


def test_mark_only_lora_trainable():
    from mfvit import lora
    m = small()
    lora.add_lora(m, freeze_base=False)
    lora.mark_only_lora_trainable(m, train_head=False)
    on = {n for n, p in m.named_parameters() if p.requires_grad}
    assert on == {n for n, _ in m.named_parameters() if "lora_" in n}
    lora.mark_only_lora_trainable(m)
    on = {n for n, p in m.named_parameters() if p.requires_grad}
    assert on == {n for n, _ in m.named_parameters() if "lora_" in n} | {"head.weight", "head.bias"}


def test_refusals():
    import types

    import vits
    from mfvit import _lib, lora
    from model.fuseattention import GPT
    for bad in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="rank"):
            lora.add_lora(small(), rank=bad)
    for bad in (("q", "w"), (), ("q", "q"), ("qkv",)):
        with pytest.raises(ValueError, match="targets"):
            lora.add_lora(small(), targets=bad)
    for bad in ([2], [-3], [0.5], []):
        with pytest.raises(ValueError, match="block"):
            lora.add_lora(small(), blocks=bad)
    m = small()
    lora.add_lora(m)
    with pytest.raises(ValueError, match="already attached"):
        lora.add_lora(m)
    for precision in ("bf16", "fp16"):
        with pytest.raises(_lib.MfvitError, match="bf16x3"):
            lora.add_lora(small(precision=precision))
    lora.add_lora(small(precision="fp32"))
    with pytest.raises(NotImplementedError):
        vits.vit_conv_small()
    args = types.SimpleNamespace(arch="vit_small", pos_embed=True)
    with pytest.raises(NotImplementedError, match="GPT"):
        lora.add_lora(GPT(384, 4, 3, 1, 2, 2, 1, 0, 0, 0, args, types.SimpleNamespace(n_views=1)))
    for fn in (lora.merge_lora, lora.remove_lora, lora.lora_state_dict, lora.mark_only_lora_trainable):
        with pytest.raises(ValueError, match="no LoRA adapters"):
            fn(small())
    assert lora.lora_parameters(small()) == []


def test_grad_sync_and_moco_builders_refuse_adapters():
    import types

    import vits
    from mfvit import lora
    from mfvit.ddp import GradSync
    from moco import builder_vit
    m = small()
    lora.add_lora(m)
    with pytest.raises(NotImplementedError, match="LoRA"):
        GradSync().attach(m)
    args = types.SimpleNamespace(arch="vit_small")
    from functools import partial
    moco = builder_vit.MoCo_ViT(partial(vits.vit_small, depth=1), args, dim=32, mlp_dim=64)
    lora.add_lora(moco.base_encoder)
    with pytest.raises(NotImplementedError, match="LoRA"):
        moco._momentum_update_key_encoder(0.99)
