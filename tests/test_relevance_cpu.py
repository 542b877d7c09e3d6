"""Class-specific attention relevance of the ViT encoders (include/mfvit.h, mfvit_vit_backward_rel; VisionTransformerMoCo.attention_relevance /
get_relevance_maps, Fus_CrossViT.attention_relevance): the host-side contract, no GPU needed.

Every C call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import importlib

import pytest
import torch

EINVAL = -22
FAKE = 1 << 20          # a non-NULL pointer value the argument checks accept (nothing is ever read from it)
METHODS = ("attention_relevance", "get_relevance_maps")
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def _lib():
    from mfvit import _lib
    return _lib


def _cfg(token_input=False, batch=2, depth=3, save=True, size=224):
    import vits
    m = vits.vit_small(num_classes=3, depth=depth, img_size=size)
    cfg = m._cfg(torch.zeros(batch, 3, size, size), save)
    if token_input:
        cfg.token_input = 1
        cfg.tokens = 64
        cfg.img_h = cfg.img_w = 0
    assert _lib().lib().mfvit_vit_workspace_bytes(cfg) > 0
    return cfg


def _req(blocks=0, maps=None, relevance=None, scratch=None):
    return _lib().VitRelReq(blocks, maps, relevance, scratch)


def test_new_symbols_are_exported_and_bound():
    L = _lib()
    h = L.lib()
    for name in ("mfvit_vit_rel_scratch_bytes", "mfvit_vit_backward_rel"):
        assert hasattr(h, name)
        assert name in L.SIGNATURES
    assert [f[0] for f in L.VitRelReq._fields_] == ["blocks", "maps", "relevance", "scratch"]
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5


@pytest.mark.parametrize("module", ["vits", "vits_returnftrs"])
@pytest.mark.parametrize("arch", ["vit_small", "vit_base", "vit_small_ori", "vit_base_ori"])
def test_every_constructor_has_the_methods(module, arch):
    m = getattr(importlib.import_module(module), arch)(num_classes=3, depth=1)
    for name in METHODS:
        assert callable(getattr(m, name)), name


def test_fus_crossvit_has_the_method():
    fus = importlib.import_module(FUS_MOD)
    assert callable(getattr(fus.Fus_CrossViT, "attention_relevance"))


INVALID = {
    "token_input": (dict(token_input=True), dict(relevance=FAKE)),
    "no_saved_activations": (dict(save=False), dict(relevance=FAKE)),
    "block_bit_at_depth": ({}, dict(blocks=1 << 3, maps=FAKE)),
    "block_bit_63": ({}, dict(blocks=1 << 63, maps=FAKE, relevance=FAKE)),
    "maps_null": ({}, dict(blocks=5, maps=None)),
    "maps_without_blocks": ({}, dict(maps=FAKE, relevance=FAKE)),
    "nothing_asked": ({}, {}),
    "tokens_over_8192": (dict(batch=1, size=1456), dict(relevance=FAKE)),      # 91 x 91 + 1 = 8282 tokens
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_requests_get_no_scratch_and_einval(case):
    cfg_kw, req_kw = INVALID[case]
    cfg, req = _cfg(**cfg_kw), _req(**req_kw)
    h = _lib().lib()
    assert h.mfvit_vit_rel_scratch_bytes(cfg, req) == 0
    req.scratch = FAKE
    assert h.mfvit_vit_backward_rel(cfg, req, FAKE, FAKE, FAKE, FAKE, None) == EINVAL


def test_valid_requests_get_scratch_and_need_scratch_and_dfeatures():
    h = _lib().lib()
    cfg = _cfg(batch=2, depth=3)
    for req in (_req(relevance=FAKE), _req(blocks=0b101, maps=FAKE), _req(blocks=0b111, maps=FAKE, relevance=FAKE)):
        assert h.mfvit_vit_rel_scratch_bytes(cfg, req) > 0
        assert h.mfvit_vit_backward_rel(cfg, req, FAKE, FAKE, FAKE, FAKE, None) == EINVAL              # scratch NULL
        req.scratch = FAKE
        assert h.mfvit_vit_backward_rel(cfg, req, FAKE, FAKE, FAKE, None, None) == EINVAL              # dfeatures NULL
    assert h.mfvit_vit_rel_scratch_bytes(cfg, None) == 0


@pytest.mark.parametrize("batch,size", [(2, 224), (128, 224), (3, 384), (1, 32)])
def test_relevance_scratch_does_not_grow_with_depth_and_is_bounded(batch, size):
    h = _lib().lib()
    T = (size // 16) ** 2 + 1
    n = [h.mfvit_vit_rel_scratch_bytes(_cfg(batch=batch, depth=d, size=size), _req(relevance=FAKE)) for d in (3, 12)]
    assert n[0] == n[1] > 0
    assert n[0] <= 4 * batch * T * ((T + 31) // 32 + 2) + 256
    assert n[0] >= 4 * batch * T * ((T + 31) // 32 + 1)                # v and the per-tile row products


@pytest.mark.parametrize("method,kw", [
    ("get_relevance_maps", dict(blocks=[2])),
    ("get_relevance_maps", dict(blocks=[0.0])),
    ("get_relevance_maps", dict(blocks=[])),
    ("attention_relevance", dict(target=3)),
    ("attention_relevance", dict(target=-1)),
    ("attention_relevance", dict(target=1.0)),
    ("attention_relevance", dict(target=True)),
    ("attention_relevance", dict(target="0")),
    ("attention_relevance", dict(target=torch.tensor([0]))),
    ("attention_relevance", dict(target=torch.tensor([[0, 1]]))),
    ("attention_relevance", dict(target=torch.tensor([0.0, 1.0]))),
    ("attention_relevance", dict(target=torch.tensor([0, 3]))),
    ("get_relevance_maps", dict(target=torch.tensor([True, False]))),
])
def test_argument_errors_raise_value_error_before_any_launch(method, kw):
    import vits
    m = vits.vit_small(num_classes=3, depth=2)
    with pytest.raises(ValueError):
        getattr(m, method)(torch.zeros(2, 3, 224, 224), **kw)


def test_fus_crossvit_target_errors_raise_value_error_before_any_launch():
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    a, b = vits.vit_small(num_classes=3, depth=1), vits.vit_small(num_classes=3, depth=1)
    model = fus.Fus_CrossViT(a, b)
    x = torch.zeros(2, 3, 224, 224)
    for t in (3, -1, 0.5, torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError):
            model.attention_relevance(a, b, x, x, target=t)
    with pytest.raises(ValueError):
        model.attention_relevance(a, b, x, x[:1])
    c = vits.vit_small(num_classes=3, depth=1)                          # not the encoder the model was built with
    for args in ((c, b), (a, c), (b, a)):
        with pytest.raises(ValueError, match="built with"):
            model.attention_relevance(*args, x, x)


def test_cpu_images_are_refused_like_forward():
    import vits
    m = vits.vit_small(num_classes=3, depth=2)
    x = torch.zeros(1, 3, 224, 224)
    for name in METHODS:
        with pytest.raises(_lib().MfvitError):
            getattr(m, name)(x)
