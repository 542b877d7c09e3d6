"""Image gradients through the ViT encoder (include/mfvit.h, mfvit_vit_backward_ex): the host-side contract, no GPU needed.

Every call below is invalid and must be refused with MFVIT_EINVAL before the library touches the GPU, so fake (never dereferenced) device
pointers are safe here."""
import ctypes

import pytest
import torch

EINVAL = -22
FAKE = 1 << 20          # a non-NULL pointer value the argument checks accept (nothing is ever read from it)


def _lib():
    from mfvit import _lib
    return _lib


def _cfg(token_input=False, save=True, batch=2, depth=3):
    import vits
    L = _lib()
    m = vits.vit_small(num_classes=3, depth=depth)
    cfg = m._cfg(torch.zeros(batch, 3, 224, 224), save)
    if token_input:
        cfg.token_input = 1
        cfg.tokens = 64
        cfg.img_h = cfg.img_w = 0
    assert L.lib().mfvit_vit_workspace_bytes(cfg) > 0
    return cfg


def _drop(depth=3, p=0.0, dpr=0.0):
    L = _lib()
    r = (ctypes.c_float * depth)(*([dpr] * depth))
    d = L.VitDrop(p, 0.0, ctypes.cast(r, ctypes.POINTER(ctypes.c_float)), 7)
    d._r = r
    return d


def _bwd_ex(cfg, drop, dparams, dimg, hi, lo):
    return _lib().lib().mfvit_vit_backward_ex(cfg, drop, FAKE, FAKE, FAKE, FAKE, dparams, dimg, hi, lo, None)


def test_new_symbols_are_exported_and_bound():
    L = _lib()
    h = L.lib()
    for name in ("mfvit_vit_workspace_bytes_ex", "mfvit_vit_backward_ex"):
        assert hasattr(h, name)
        assert name in L.SIGNATURES
    assert h.mfvit_abi_version() == L.ABI_VERSION == 5


def test_dimg_in_token_input_mode_is_rejected():
    cfg = _cfg(token_input=True)
    assert _bwd_ex(cfg, None, FAKE, FAKE, cfg.depth, -1) == EINVAL
    assert _bwd_ex(cfg, None, None, FAKE, cfg.depth, -1) == EINVAL


@pytest.mark.parametrize("lo", [0, 1, 3])
def test_dimg_needs_the_embedding_stage(lo):
    cfg = _cfg()
    assert _bwd_ex(cfg, None, FAKE, FAKE, cfg.depth, lo) == EINVAL
    assert _bwd_ex(cfg, None, None, FAKE, cfg.depth, lo) == EINVAL
    assert _bwd_ex(cfg, _drop(p=0.1), None, FAKE, cfg.depth, lo) == EINVAL


def test_no_dimg_and_no_dparams_is_rejected():
    cfg = _cfg()
    assert _bwd_ex(cfg, None, None, None, cfg.depth, -1) == EINVAL
    assert _bwd_ex(cfg, _drop(dpr=0.1), None, None, cfg.depth, -1) == EINVAL


def test_the_old_entry_points_still_refuse_null_dparams():
    cfg = _cfg()
    h = _lib().lib()
    assert h.mfvit_vit_backward(cfg, FAKE, FAKE, FAKE, FAKE, None, cfg.depth, -1, None) == EINVAL
    assert h.mfvit_vit_backward_drop(cfg, _drop(), FAKE, FAKE, FAKE, FAKE, None, cfg.depth, -1, None) == EINVAL


def test_backward_without_saved_activations_is_rejected():
    cfg = _cfg(save=False)
    assert _bwd_ex(cfg, None, FAKE, FAKE, cfg.depth, -1) == EINVAL


def test_workspace_bytes_ex():
    L = _lib()
    h = L.lib()
    cfg = _cfg()
    base = h.mfvit_vit_workspace_bytes(cfg)
    assert h.mfvit_vit_workspace_bytes_ex(cfg, None, 0) == base
    ex = h.mfvit_vit_workspace_bytes_ex(cfg, None, 1)
    assert ex >= base + 768 * 384 * 4                       # W_pe^T (split bf16: 4 bytes per element) behind the usual layout
    d = _drop(dpr=0.1)
    assert h.mfvit_vit_workspace_bytes_ex(cfg, d, 0) == h.mfvit_vit_workspace_bytes_drop(cfg, d)
    assert h.mfvit_vit_workspace_bytes_ex(cfg, d, 1) > h.mfvit_vit_workspace_bytes_drop(cfg, d)
    # invalid configurations: 0
    assert h.mfvit_vit_workspace_bytes_ex(cfg, _drop(p=1.0), 1) == 0
    assert h.mfvit_vit_workspace_bytes_ex(_cfg(token_input=True), None, 1) == 0
    assert h.mfvit_vit_workspace_bytes_ex(_cfg(save=False), None, 1) == 0
    bad = _cfg()
    bad.img_w = 230
    assert h.mfvit_vit_workspace_bytes_ex(bad, None, 0) == h.mfvit_vit_workspace_bytes_ex(bad, None, 1) == 0
    bad = _cfg()
    bad.dim = 512
    assert h.mfvit_vit_workspace_bytes_ex(bad, None, 1) == 0
    f32 = _cfg()
    f32.dtype = L.F32
    assert h.mfvit_vit_workspace_bytes_ex(f32, _drop(p=0.1), 1) == 0                # fp32: no dropout stages
    assert h.mfvit_vit_workspace_bytes_ex(f32, None, 1) > h.mfvit_vit_workspace_bytes(f32)


@pytest.mark.parametrize("frozen", [False, True])
def test_cpu_images_that_require_a_gradient_still_raise(frozen):
    import vits
    L = _lib()
    m = vits.vit_small(num_classes=3, depth=2)
    if frozen:
        for p in m.parameters():
            p.requires_grad = False
    img = torch.zeros(1, 3, 224, 224, requires_grad=True)
    with pytest.raises(L.MfvitError):
        m(img)
    with pytest.raises(L.MfvitError):
        m.features3D(img)
