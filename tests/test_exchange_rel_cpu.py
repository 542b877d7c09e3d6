"""Exchange attention maps and cross-stream relevance of Fus_CrossViT (include/mfvit.h: mfvit_fusion_ex_attention, mfvit_fusion_ex_grad_attention,
mfvit_bimodal_relevance; Fus_CrossViT.get_exchange_attention / exchange_relevance / cross_relevance): what can be checked without a GPU.

  * the vector-chain form the GPU kernel runs equals the explicit T x T definition (tests/exchange_rel_ref.py) to 1e-12;
  * mutations of the definition move the result by far more than any gate of tests/test_exchange_rel_gpu.py, so those gates can see them;
  * the Python argument checks raise before anything is launched, the C entry points refuse invalid arguments before any HIP call (fake, never
    dereferenced device pointers are safe), and the new symbols are exported and bound."""
import importlib

import pytest
import torch

import exchange_rel_ref as R

EINVAL = -22
FAKE = 1 << 20
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
LOOSEST_GPU_GATE = 1e-3          # TOL["bf16x3"], the ceiling of check 4 of the GPU tests; checks 1 - 3 are at most 1e-5


def _inputs(seed, T=13, B=2, Lc=3, Le=2, zero_c=None, zero_e=None):
    A_c = R.synthetic_maps(seed, Lc, B, T, zero_token=zero_c)
    A_e = R.synthetic_maps(seed + 1, Le, B, T, zero_token=zero_e)
    g = torch.Generator().manual_seed(seed + 2)
    per_head = torch.rand(2, B, 6, T, generator=g, dtype=torch.float64) * 0.2        # max(0, a_h da_h) of 6 heads, both directions
    return A_c, A_e, per_head


# zero_c / zero_e: a token whose rows are zero in every map of that stream (n = 0: its Rbar row is e_j); token 0 is the cls token (Rbar[0,0] = 1)
@pytest.mark.parametrize("zero_c,zero_e", [(None, None), (4, 7), (0, None), (None, 0)])
def test_chain_form_equals_the_explicit_matrix_form(zero_c, zero_e):
    A_c, A_e, ph = _inputs(11, zero_c=zero_c, zero_e=zero_e)
    ab = ph.mean(dim=2)
    want = R.explicit_cross_relevance(A_c, A_e, ab[0], ab[1])
    got = R.chain_cross_relevance(A_c, A_e, ab[0], ab[1])
    assert all(float(w.abs().max()) > 0 for w in want[1:3])
    for g, w in zip(got, want):
        assert g.shape == w.shape == (2, 12)
        assert R.rel_err(g, w) < 1e-12


def test_zero_row_token_keeps_its_own_weight_only():
    A_c, A_e, ph = _inputs(12, zero_e=5)
    ab = ph.mean(dim=2)
    _, rel_ce, _, _ = R.explicit_cross_relevance(A_c, A_e, ab[0], ab[1])
    # token 5 of the ENH stream has Rbar row e_5: it passes w[5] to itself and receives nothing from it through the other rows' chains
    A0 = [a.clone() for a in A_e]
    ab0 = ab.clone()
    ab0[0, :, 5] = 0
    _, without, _, _ = R.explicit_cross_relevance(A_c, A0, ab0[0], ab[1])
    d = rel_ce - without
    assert torch.allclose(d[:, :4], torch.zeros_like(d[:, :4]), atol=1e-15) and torch.allclose(d[:, 5:], torch.zeros_like(d[:, 5:]), atol=1e-15)
    assert float(d[:, 4].abs().min()) > 0


@pytest.mark.parametrize("mutation,moved", [("no_normalisation", (1, 2)), ("no_own_cls_term", (0, 3)), ("swapped_directions", (0, 1, 2, 3)),
                                            ("one_head_dropped", (0, 1, 2, 3))])
def test_mutations_move_the_result_by_more_than_the_gpu_gates(mutation, moved):
    A_c, A_e, ph = _inputs(13)
    ab = ph.mean(dim=2)
    want = R.explicit_cross_relevance(A_c, A_e, ab[0], ab[1])
    if mutation == "no_normalisation":
        got = R.chain_cross_relevance(A_c, A_e, ab[0], ab[1], normalise=False)
    elif mutation == "no_own_cls_term":
        got = R.chain_cross_relevance(A_c, A_e, ab[0], ab[1], own_cls_term=False)
    elif mutation == "swapped_directions":
        got = R.chain_cross_relevance(A_c, A_e, ab[0], ab[1], swap=True)
    else:
        ab1 = ph[:, :, :-1].sum(dim=2) / ph.shape[2]
        got = R.chain_cross_relevance(A_c, A_e, ab1[0], ab1[1])
    for k in moved:
        assert R.rel_err(got[k], want[k]) > 10 * LOOSEST_GPU_GATE, (mutation, k)


def test_abar_of_is_the_head_mean_of_the_clamped_products():
    a = torch.rand(2, 6, 1, 9, dtype=torch.float64).requires_grad_(True)
    b = a * 1.0
    b.retain_grad()
    wgt = torch.randn(2, 6, 1, 9, dtype=torch.float64)
    (b * wgt).sum().backward()
    want = (a.detach() * wgt).clamp(min=0)[:, :, 0].mean(dim=1)
    assert torch.allclose(R.abar_of(b), want, atol=0, rtol=1e-15)
    assert R.rel_err(R.abar_of(b, drop_last_head=True), want) > 10 * LOOSEST_GPU_GATE


# ------------------------------------------------------------------------------------------------ the library boundary
def _lib():
    from mfvit import _lib
    return _lib


def test_new_symbols_are_exported_and_bound():
    L = _lib()
    h = L.lib()
    for name in ("mfvit_fusion_ex_attention", "mfvit_fusion_ex_grad_attention", "mfvit_bimodal_relevance", "mfvit_bimodal_relevance_scratch_bytes"):
        assert hasattr(h, name)
        assert name in L.SIGNATURES
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5


def _fcfg(T=197, heads=3, dim=384, B=2):
    from mfvit.fusion import fusion_cfg
    return fusion_cfg(B, T, 3, dim, heads)


def test_exchange_map_entry_points_refuse_invalid_arguments_before_any_hip_call():
    h = _lib().lib()
    ok = _fcfg()
    att, gat = h.mfvit_fusion_ex_attention, h.mfvit_fusion_ex_grad_attention
    assert att(ok, 1, 0, None, 0, 0, FAKE, None) == EINVAL                       # workspace NULL
    assert att(ok, 1, 0, FAKE, 0, 0, None, None) == EINVAL                       # out NULL
    assert att(None, 1, 0, FAKE, 0, 0, FAKE, None) == EINVAL
    for layer, depth in ((-1, 1), (1, 1), (2, 2), (3, 2)):
        assert att(ok, depth, 0, FAKE, layer, 0, FAKE, None) == EINVAL
        assert gat(ok, depth, 0, FAKE, FAKE, FAKE, FAKE, layer, FAKE, None) == EINVAL
    for fuse in (-1, 4):
        assert att(ok, 1, 0, FAKE, 0, fuse, FAKE, None) == EINVAL
    big = _fcfg(T=8193)
    assert att(big, 1, 0, FAKE, 0, 0, FAKE, None) == EINVAL
    assert gat(big, 1, 0, FAKE, FAKE, FAKE, FAKE, 0, FAKE, None) == EINVAL
    assert att(_fcfg(heads=4), 1, 0, FAKE, 0, 0, FAKE, None) == EINVAL           # (the checks of mfvit_fusion_ex_forward)
    assert att(ok, 17, 0, FAKE, 0, 0, FAKE, None) == EINVAL
    for i in range(5):                                                           # params, f_cxr, f_enh, workspace, abar NULL
        args = [FAKE] * 5
        args[i] = None
        assert gat(ok, 1, 0, args[0], args[1], args[2], args[3], 0, args[4], None) == EINVAL


def test_bimodal_relevance_refuses_invalid_arguments_before_any_hip_call():
    h = _lib().lib()
    f, sb = h.mfvit_bimodal_relevance, h.mfvit_bimodal_relevance_scratch_bytes
    assert sb(2, 197) >= 2 * 2 * 4 and sb(128, 8192) >= 2 * 128 * 4
    for B, T in ((0, 197), (2, 1), (2, 8193), (-1, 5)):
        assert sb(B, T) == 0
        assert f(B, T, 2, 2, FAKE, FAKE, FAKE, FAKE, FAKE, None) == EINVAL
    for dc, de in ((0, 2), (2, 0), (-1, 1)):
        assert f(2, 197, dc, de, FAKE, FAKE, FAKE, FAKE, FAKE, None) == EINVAL
    for i in range(5):                                                           # maps_c, maps_e, abar, out4, scratch NULL
        args = [FAKE] * 5
        args[i] = None
        assert f(2, 197, 2, 2, *args, None) == EINVAL


# ------------------------------------------------------------------------------------------------ the Python surface
def _model(**kw):
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    a, b = vits.vit_small(num_classes=3, depth=1), vits.vit_small(num_classes=3, depth=1)
    return fus.Fus_CrossViT(a, b, **kw), a, b, vits


def test_fus_crossvit_has_the_methods():
    fus = importlib.import_module(FUS_MOD)
    for name in ("get_exchange_attention", "exchange_relevance", "cross_relevance"):
        assert callable(getattr(fus.Fus_CrossViT, name))


@pytest.mark.parametrize("method", ["get_exchange_attention", "exchange_relevance", "cross_relevance"])
def test_wrong_encoders_and_batch_mismatch_raise_value_error_before_any_launch(method):
    model, a, b, vits = _model()
    x = torch.zeros(2, 3, 224, 224)
    with pytest.raises(ValueError):
        getattr(model, method)(a, b, x, x[:1])
    with pytest.raises(ValueError):
        getattr(model, method)(a, b, x, None)
    c = vits.vit_small(num_classes=3, depth=1)                          # not the encoder the model was built with
    for args in ((c, b), (a, c), (b, a)):
        with pytest.raises(ValueError, match="built with"):
            getattr(model, method)(*args, x, x)


@pytest.mark.parametrize("method", ["exchange_relevance", "cross_relevance"])
def test_target_errors_raise_value_error_before_any_launch(method):
    model, a, b, _ = _model()
    x = torch.zeros(2, 3, 224, 224)
    for t in (3, -1, 0.5, True, "0", torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0]), torch.tensor([0, 3])):
        with pytest.raises(ValueError):
            getattr(model, method)(a, b, x, x, target=t)


def test_head_fusion_errors_raise_value_error_before_any_launch():
    model, a, b, _ = _model()
    x = torch.zeros(2, 3, 224, 224)
    for hf in ("avg", "sum", 1, 0):
        with pytest.raises(ValueError, match="head_fusion"):
            model.get_exchange_attention(a, b, x, x, head_fusion=hf)


@pytest.mark.parametrize("kw", [dict(cross_attn_depth=2), dict(pool="mean"), dict(cross_attn_depth=3, pool="mean")])
@pytest.mark.parametrize("method", ["exchange_relevance", "cross_relevance"])
def test_relevance_beyond_one_layer_cls_is_not_implemented(method, kw):
    model, a, b, _ = _model(**kw)
    x = torch.zeros(2, 3, 224, 224)
    with pytest.raises(NotImplementedError):
        getattr(model, method)(a, b, x, x)
    with pytest.raises(ValueError):                                     # argument errors still come first
        getattr(model, method)(a, b, x, x, target=7)


@pytest.mark.parametrize("method", ["get_exchange_attention", "exchange_relevance", "cross_relevance"])
def test_cpu_images_are_refused_like_forward(method):
    model, a, b, _ = _model()
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(_lib().MfvitError):
        getattr(model, method)(a, b, x, x)
