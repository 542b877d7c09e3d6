"""Fus_CrossViT beyond the default shape, host side: construction, state-dict keys against the reference's
(tests/golden/fusion_ex_keys.npz, tools/make_fusion_ex_golden.py), argument checks and the _ex C ABI's arena size."""
import importlib

import pytest

FUS_MOD = ("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
           "changemodelinputlocation_std002_sum")
KEY_CASES = [("dim768", dict(small_dim=768, large_dim=768)), ("L2", dict(cross_attn_depth=2)), ("M2", dict(multi_scale_enc_depth=2)),
             ("mean", dict(pool="mean"))]


def _vits():
    import vits_returnftrs as vits
    return vits.vit_small(num_classes=3), vits.vit_small(num_classes=3)


@pytest.mark.parametrize("name,kw", KEY_CASES)
def test_constructs_with_reference_keys(golden, name, kw):
    fus = importlib.import_module(FUS_MOD)
    model = fus.Fus_CrossViT(*_vits(), **kw)
    assert sorted(model.state_dict().keys()) == list(golden("fusion_ex_keys.npz")[name])
    assert model._arena.intact()


@pytest.mark.parametrize("kw,exc", [(dict(small_dim=384, large_dim=768), ValueError), (dict(heads=4), NotImplementedError),
                                    (dict(heads=8), NotImplementedError), (dict(small_dim=512, large_dim=512), NotImplementedError),
                                    (dict(dropout=0.1), NotImplementedError), (dict(pool="max"), ValueError)])
def test_unsupported_arguments_raise(kw, exc):
    fus = importlib.import_module(FUS_MOD)
    with pytest.raises(exc):
        fus.Fus_CrossViT(*_vits(), **kw)


def test_heads_error_names_the_supported_set():
    fus = importlib.import_module(FUS_MOD)
    with pytest.raises(NotImplementedError, match=r"\(3, 6, 12\)"):
        fus.MultiScaleTransformerEncoder(cross_attn_heads=4)


@pytest.mark.parametrize("dim,heads,L,pool,M", [(384, 3, 1, "cls", 1), (384, 3, 2, "cls", 1), (384, 3, 1, "mean", 1), (768, 3, 1, "cls", 1),
                                                (768, 12, 2, "mean", 2), (384, 6, 3, "cls", 3)])
def test_ex_param_count_is_the_arena_tail(dim, heads, L, pool, M):
    from mfvit import _lib
    from mfvit.fusion import fusion_cfg
    fus = importlib.import_module(FUS_MOD)
    model = fus.Fus_CrossViT(*_vits(), small_dim=dim, large_dim=dim, cross_attn_depth=L, multi_scale_enc_depth=M, heads=heads, pool=pool)
    flat = model.flat_parameters()
    tail, off = model._spec.tail(flat)
    assert _lib.lib().mfvit_fusion_ex_param_count(fusion_cfg(4, 197, 3, dim, heads), L, int(pool == "mean")) == tail.numel()
    dead = sum(p.numel() for n, p in model.named_parameters() if not n.startswith(f"multi_scale_transformers.{M - 1}.")
               and n.startswith("multi_scale_transformers."))
    assert off == dead
    assert [id(p) for p in model._spec.live()] == [id(p) for n, p in model.named_parameters() if n not in
                                                   {n2 for n2, _ in model.named_parameters() if n2.startswith("multi_scale_transformers.")
                                                    and not n2.startswith(f"multi_scale_transformers.{M - 1}.")}]


def test_ex_abi_rejects_invalid_configurations():
    from mfvit import _lib
    from mfvit.fusion import fusion_cfg
    lib = _lib.lib()
    assert lib.mfvit_fusion_ex_workspace_bytes(fusion_cfg(4, 197, 3, 384, 3), 2, 1) > 0
    assert lib.mfvit_fusion_ex_workspace_bytes(fusion_cfg(4, 197, 3, 384, 3), 1, 0) == lib.mfvit_fusion_workspace_bytes(fusion_cfg(4, 197, 3))
    for cfg, L, pm in [(fusion_cfg(4, 197, 3, 512, 4), 1, 0), (fusion_cfg(4, 197, 3, 384, 4), 1, 0), (fusion_cfg(4, 197, 3), 0, 0),
                       (fusion_cfg(4, 197, 3), 17, 0), (fusion_cfg(4, 197, 3), 1, 2), (fusion_cfg(0, 197, 3), 2, 0)]:
        assert lib.mfvit_fusion_ex_workspace_bytes(cfg, L, pm) == 0
        assert lib.mfvit_fusion_ex_param_count(cfg, L, pm) == 0
    assert lib.mfvit_fusion_param_count(fusion_cfg(4, 197, 3, 768, 12)) == 8 * 768 * 768 + 10 * 768 + 2 * (3 * 768 + 3)
    assert lib.mfvit_fusion_ex_forward(fusion_cfg(4, 197, 3), 0, 0, *([None] * 12)) == lib.mfvit_fusion_ex_backward(
        fusion_cfg(4, 197, 3), 0, 0, *([None] * 17)) != 0
