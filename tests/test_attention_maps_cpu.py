"""Attention maps of the ViT encoders (include/mfvit.h, mfvit_vit_forward_attn; VisionTransformerMoCo.get_attention_maps /
get_last_selfattention / attention_rollout): the host-side contract, no GPU needed.

Every C call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import pytest
import torch

EINVAL = -22
FAKE = 1 << 20          # a non-NULL pointer value the argument checks accept (nothing is ever read from it)
METHODS = ("get_attention_maps", "get_last_selfattention", "attention_rollout")


def _lib():
    from mfvit import _lib
    return _lib


def _cfg(token_input=False, batch=2, depth=3):
    import vits
    m = vits.vit_small(num_classes=3, depth=depth)
    cfg = m._cfg(torch.zeros(batch, 3, 224, 224), False)
    if token_input:
        cfg.token_input = 1
        cfg.tokens = 64
        cfg.img_h = cfg.img_w = 0
    assert _lib().lib().mfvit_vit_workspace_bytes(cfg) > 0
    return cfg


def _req(blocks=0, fuse=0, cls_only=0, maps=None, rollout=None, scratch=None):
    return _lib().VitAttnReq(blocks, fuse, cls_only, maps, rollout, scratch)


def test_new_symbols_are_exported_and_bound():
    L = _lib()
    h = L.lib()
    for name in ("mfvit_vit_attn_scratch_bytes", "mfvit_vit_forward_attn"):
        assert hasattr(h, name)
        assert name in L.SIGNATURES
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5


@pytest.mark.parametrize("module", ["vits", "vits_returnftrs"])
@pytest.mark.parametrize("arch", ["vit_small", "vit_base", "vit_small_ori", "vit_base_ori"])
def test_every_constructor_has_the_methods(module, arch):
    import importlib
    m = getattr(importlib.import_module(module), arch)(num_classes=3, depth=1)
    for name in METHODS:
        assert callable(getattr(m, name)), name


INVALID = {
    "token_input": (dict(token_input=True), dict(blocks=1, maps=FAKE)),
    "block_bit_at_depth": ({}, dict(blocks=1 << 3, maps=FAKE)),
    "block_bit_63": ({}, dict(blocks=1 << 63, maps=FAKE)),
    "fuse_negative": ({}, dict(blocks=1, fuse=-1, maps=FAKE)),
    "fuse_4": ({}, dict(blocks=1, fuse=4, maps=FAKE)),
    "cls_only_2": ({}, dict(blocks=1, cls_only=2, maps=FAKE)),
    "rollout_per_head": ({}, dict(rollout=FAKE)),
    "maps_null": ({}, dict(blocks=5, fuse=1, maps=None)),
    "maps_without_blocks": ({}, dict(fuse=1, maps=FAKE, rollout=FAKE)),
    "nothing_asked": ({}, dict(fuse=1)),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_requests_get_no_scratch_and_einval(case):
    cfg_kw, req_kw = INVALID[case]
    cfg, req = _cfg(**cfg_kw), _req(**req_kw)
    h = _lib().lib()
    assert h.mfvit_vit_attn_scratch_bytes(cfg, req) == 0
    req.scratch = FAKE
    assert h.mfvit_vit_forward_attn(cfg, req, FAKE, FAKE, FAKE, FAKE, FAKE, None) == EINVAL


def test_valid_requests_get_scratch_and_need_it():
    h = _lib().lib()
    cfg = _cfg(batch=2, depth=3)
    T = 197
    for req in (_req(blocks=0b101, maps=FAKE), _req(blocks=1, fuse=2, cls_only=1, maps=FAKE), _req(fuse=1, rollout=FAKE),
                _req(blocks=0b111, fuse=3, maps=FAKE, rollout=FAKE)):
        n = h.mfvit_vit_attn_scratch_bytes(cfg, req)
        assert n > 0
        if req.rollout:     # the depth fused maps and their row sums
            assert n >= 3 * 2 * T * (T + 1) * 4
        assert h.mfvit_vit_forward_attn(cfg, req, FAKE, FAKE, FAKE, FAKE, FAKE, None) == EINVAL     # scratch NULL
    assert h.mfvit_vit_attn_scratch_bytes(cfg, None) == 0


@pytest.mark.parametrize("method,kw", [
    ("get_attention_maps", dict(head_fusion="avg")),
    ("get_attention_maps", dict(head_fusion="MEAN")),
    ("get_attention_maps", dict(blocks=[2])),
    ("get_attention_maps", dict(blocks=[0, -3])),
    ("get_attention_maps", dict(blocks=[0.0])),
    ("get_attention_maps", dict(blocks=[True])),
    ("get_attention_maps", dict(blocks=[])),
    ("attention_rollout", dict(head_fusion=None)),
    ("attention_rollout", dict(head_fusion="sum")),
])
def test_argument_errors_raise_value_error_before_any_launch(method, kw):
    import vits
    m = vits.vit_small(num_classes=3, depth=2)
    with pytest.raises(ValueError):
        getattr(m, method)(torch.zeros(1, 3, 224, 224), **kw)


def test_cpu_images_are_refused_like_forward():
    import vits
    m = vits.vit_small(num_classes=3, depth=2)
    x = torch.zeros(1, 3, 224, 224)
    for name in METHODS:
        with pytest.raises(_lib().MfvitError):
            getattr(m, name)(x)
