"""timm regularisation kwargs of the ViT encoder (drop_rate, attn_drop_rate, drop_path_rate): host-side plumbing, no GPU needed."""
import pytest
import torch


def _vits():
    import vits
    return vits


def test_kwargs_reach_the_rate_carrier_modules_and_dpr_is_timms_linspace():
    vits = _vits()
    m = vits.vit_small(num_classes=3, depth=5, drop_rate=0.1, attn_drop_rate=0.05, drop_path_rate=0.2)
    assert m.pos_drop.p == 0.1
    for b in m.blocks:
        assert b.attn.attn_drop.p == 0.05 and b.attn.proj_drop.p == 0.1 and b.mlp.drop.p == 0.1
    dpr = [x.item() for x in torch.linspace(0, 0.2, 5)]
    assert isinstance(m.blocks[0].drop_path, torch.nn.Identity)           # timm 0.4.9: block 0 gets rate 0 -> Identity
    assert [getattr(b.drop_path, "drop_prob", 0.0) for b in m.blocks] == dpr
    drop, attn, rates = m.drop_rates()
    assert (drop, rates) == (pytest.approx(0.1), dpr) and attn == pytest.approx(0.05)
    mb = vits.vit_base(num_classes=3, depth=3, drop_path_rate=0.1)
    assert [getattr(b.drop_path, "drop_prob", 0.0) for b in mb.blocks] == [x.item() for x in torch.linspace(0, 0.1, 3)]


def test_state_dict_keys_and_arena_are_the_same_with_and_without_rates():
    vits = _vits()
    a = vits.vit_small(num_classes=3, depth=2)
    b = vits.vit_small(num_classes=3, depth=2, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert [n for n, _ in a.arena_named_parameters()] == [n for n, _ in b.arena_named_parameters()]
    assert a.flat_parameters().numel() == b.flat_parameters().numel()
    b.load_state_dict(a.state_dict(), strict=True)


@pytest.mark.parametrize("kw", [{"drop_rate": 1.0}, {"attn_drop_rate": -0.1}, {"drop_path_rate": 1.5}])
def test_rates_outside_the_unit_interval_raise(kw):
    with pytest.raises(ValueError):
        _vits().vit_small(num_classes=3, depth=2, **kw)


def test_other_unknown_timm_kwargs_are_still_accepted():
    m = _vits().vit_small(num_classes=3, depth=2, norm_layer=None, representation_size=None)
    assert not m.is_stochastic()


def test_training_mode_with_a_rate_is_stochastic_and_eval_is_not():
    vits = _vits()
    m = vits.vit_small(num_classes=3, depth=2, drop_path_rate=0.1)
    assert m.training and m.is_stochastic()
    m.eval()
    assert not m.is_stochastic() and m._draw_drop() is None
    z = vits.vit_small(num_classes=3, depth=2)
    assert z.training and not z.is_stochastic() and z._draw_drop() is None


def test_seed_comes_from_torchs_generator():
    m = _vits().vit_small(num_classes=3, depth=3, drop_rate=0.1, drop_path_rate=0.1, precision="bf16x3")
    torch.manual_seed(5)
    d1 = m._draw_drop()
    torch.manual_seed(5)
    d2 = m._draw_drop()
    d3 = m._draw_drop()
    assert d1.seed == d2.seed != d3.seed
    assert [d1.drop_path[i] for i in range(3)] == pytest.approx([0.0, 0.05, 0.1])


def test_fp32_refuses_dropout_in_training_mode():
    from mfvit import _lib
    m = _vits().vit_small(num_classes=3, depth=2, drop_rate=0.1, precision="fp32")
    with pytest.raises(_lib.MfvitError, match="fp32"):
        m._draw_drop()
    m.eval()
    assert m._draw_drop() is None                     # evaluation runs no dropout: fp32 is fine there


def test_c_abi_drop_struct_validation_and_workspace():
    import ctypes
    from mfvit import _lib
    lib = _lib.lib()
    m = _vits().vit_small(num_classes=3, depth=3)
    cfg = m._cfg(torch.zeros(2, 3, 224, 224), True)

    def drop(p=0.0, pa=0.0, dpr=(0.0, 0.0, 0.0)):
        r = (ctypes.c_float * 3)(*dpr)
        d = _lib.VitDrop(p, pa, ctypes.cast(r, ctypes.POINTER(ctypes.c_float)), 7)
        d._r = r
        return d
    base = lib.mfvit_vit_workspace_bytes(cfg)
    assert base > 0
    assert lib.mfvit_vit_workspace_bytes_drop(cfg, drop()) == base                  # rates 0: today's layout
    assert lib.mfvit_vit_workspace_bytes_drop(cfg, drop(pa=0.1)) == base            # attention dropout needs no scratch
    assert lib.mfvit_vit_workspace_bytes_drop(cfg, drop(dpr=(0.0, 0.05, 0.1))) > base   # masked branches: one scratch row block
    assert lib.mfvit_vit_workspace_bytes_drop(cfg, drop(p=1.0)) == 0
    assert lib.mfvit_vit_workspace_bytes_drop(cfg, drop(dpr=(0.0, 1.0, 0.0))) == 0
    cfg.dtype = _lib.F32
    assert lib.mfvit_vit_workspace_bytes_drop(cfg, drop(p=0.1)) == 0               # fp32: no dropout stages
    assert lib.mfvit_vit_workspace_bytes_drop(cfg, drop()) == lib.mfvit_vit_workspace_bytes(cfg)
