"""CPU checks of patch dropout (timm PatchDropout): the float64 restatement tests/patch_drop_ref.py against the unchanged oracle, the rule for
K and the draw, the restatement's own float32 error on the inputs of the GPU tests (a tenth of the fp32 gates: the reference alone cannot fail
them), wrong variants of the restatement that the gates must catch (ten times the gates, on those same inputs), and the host surface."""
import ctypes
import os
import re

import pytest
import torch

import patch_drop_ref as R
from mfvit import _lib
from mfvit._lib import MfvitError
from oracle import ref_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP_F, CAP_G = R.CAPS["fp32"]
NEW_SYMBOLS = ["mfvit_vit_workspace_bytes_x0", "mfvit_vit_forward_x0", "mfvit_vit_backward_x0", "mfvit_patch_keep_workspace_bytes",
               "mfvit_patch_keep_embed", "mfvit_patch_keep_embed_bwd"]


def test_all_patches_kept_is_the_oracle_encoder_exactly():
    for hw, depth, B in (((64, 64), 2, 2), ((96, 64), 1, 3)):
        p = {k: v.double() for k, v in R.params_for(7001, hw, depth).items()}
        img = R.rng(7002, (B, 3) + hw).double()
        L = (hw[0] // 16) * (hw[1] // 16)
        idx = torch.arange(L).expand(B, L)
        assert torch.equal(R.features3d_keep(p, img, idx), ref_vit.features3d(p, img))


def test_number_of_kept_patches_and_the_draw():
    assert [R.num_keep(196, r) for r in (0.25, 0.5, 0.75, 0.999, 0.0)] == [147, 98, 49, 1, 196]
    from mfvit.encoder import PatchDropout
    for rate, K in ((0.25, 147), (0.5, 98), (0.75, 49), (0.999, 1)):
        pd = PatchDropout(rate)
        assert pd.num_keep(196) == K
        torch.manual_seed(3)
        a = pd.draw(4, 196, "cpu")
        torch.manual_seed(3)
        b, c = pd.draw(4, 196, "cpu"), pd.draw(4, 196, "cpu")
        torch.manual_seed(3)
        d = R.draw_indices(4, 196, rate)
        assert a.shape == (4, K) and a.dtype == torch.int64 and torch.equal(a, b) and torch.equal(a, d)       # timm's draw, reproducible
        assert K == 1 or not torch.equal(b, c)
        assert int(a.min()) >= 0 and int(a.max()) < 196 and all(len(set(r)) == K for r in a.tolist())
    po = PatchDropout(0.5, ordered=True)
    torch.manual_seed(4)
    o = po.draw(3, 24, "cpu")
    torch.manual_seed(4)
    u = PatchDropout(0.5).draw(3, 24, "cpu")
    assert torch.equal(o, u.sort(dim=-1)[0]) and not torch.equal(o, u)
    assert "prob=0.5" in repr(po) and "ordered=True" in repr(po)


@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_restatement_stays_within_a_tenth_of_the_fp32_gates(name):
    """On the inputs of the GPU tests the float32 evaluation of the restatement differs from the float64 one by less than a tenth of the fp32
    gates: the reference's own rounding cannot fail a GPU gate, and none of the inputs is ill-conditioned."""
    p, img, idx, r, rl = R.case_inputs(name)
    grads = R.CASES[name][5]
    ref = R.reference(name)
    got = R.run(p, img, idx, r, rl, torch.float32, grads=grads)
    errs = {"features": R.scale_err(got["features"], ref["features"]), "logits": R.scale_err(got["logits"], ref["logits"])}
    assert errs["features"] < CAP_F / 10 and errs["logits"] < CAP_F / 10, errs
    if grads:
        for k, g in ref["grads"].items():
            errs[k] = R.scale_err(got["grads"][k], g)
        errs["dimg"] = R.scale_err(got["dimg"], ref["dimg"])
        assert "pos_embed" not in ref["grads"]
        assert max(errs.values()) < CAP_G / 10, {k: v for k, v in errs.items() if v >= CAP_G / 10}
        # the reference itself leaves the dropped patches of d img at exact zero
        hw = R.CASES[name][0]
        assert bool((ref["dimg"][R.dropped_mask(idx, hw).expand_as(ref["dimg"])] == 0).all())


@pytest.mark.parametrize("name,mutation", [("sq64", "pos_after_gather"), ("sq64", "sample0_indices"), ("rect96x64", "pos_after_gather"),
                                           ("rect96x64", "sample0_indices"), ("rect96x64", "row_col_swapped"), ("k64", "pos_after_gather"),
                                           ("k64", "sample0_indices")])
def test_wrong_restatements_exceed_the_gates_tenfold(name, mutation):
    p, img, idx, r, rl = R.case_inputs(name)
    ref = R.reference(name)
    got = R.run(p, img, idx, r, rl, torch.float64, fn=R.MUTATIONS[mutation])
    e_f, e_d = R.scale_err(got["features"], ref["features"]), R.scale_err(got["dimg"], ref["dimg"])
    worst = max(R.scale_err(got["grads"][k], g) for k, g in ref["grads"].items())
    assert e_f > 10 * CAP_F and e_d > 10 * CAP_G and worst > 10 * CAP_G, (e_f, e_d, worst)
    for prec, (cf, cg) in R.CAPS.items():      # (and no precision's own, wider gate lets the mutation through)
        assert e_f > 3 * cf and e_d > 3 * cg, (prec, e_f, e_d)


@pytest.mark.parametrize("name", ["sq64", "rect96x64", "t2", "k195"])
def test_unzeroed_dropped_patches_exceed_the_gate_tenfold(name):
    _, _, idx, _, _ = R.case_inputs(name)
    ref = R.reference(name)
    e = R.scale_err(R.dimg_not_zeroed(ref["dimg"], idx), ref["dimg"])
    assert e > 10 * max(cg for _, cg in R.CAPS.values()), e
    full = torch.arange(16).expand(2, 16)
    d = R.rng(1, (2, 3, 64, 64))
    assert torch.equal(R.dimg_not_zeroed(d, full), d)           # nothing dropped: nothing to fill


# --------------------------------------------------------------------------------------------------- host surface
def test_constructor_keeps_the_rate():
    import vits
    import vits_returnftrs
    m = vits.vit_small(depth=1, num_classes=3, patch_drop_rate=0.5)
    assert m.patch_drop.prob == 0.5 and m.patch_drop.ordered is False and m.patch_drop.num_prefix_tokens == 1
    assert "PatchDropout(prob=0.5" in repr(m)
    mo = vits_returnftrs.vit_small(depth=1, num_classes=3, patch_drop_rate=0.25, patch_drop_ordered=True, img_size=(96, 64))
    assert mo.patch_drop.prob == 0.25 and mo.patch_drop.ordered is True
    assert vits.vit_small(depth=1).patch_drop.prob == 0.0
    assert list(m.state_dict()) == list(vits.vit_small(depth=1, num_classes=3).state_dict())      # a rate carrier: no parameter, no buffer
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            vits.vit_small(depth=1, patch_drop_rate=bad)


def test_which_forwards_drop_patches():
    import vits
    m = vits.vit_small(depth=1, num_classes=3, patch_drop_rate=0.5, img_size=64)
    x = torch.zeros(2, 3, 64, 64)
    assert m.training and m.is_stochastic()
    torch.manual_seed(1)
    i = m._resolve_keep(x, None)
    assert i.shape == (2, 8)
    with m.pinned_keep_indices(i):
        assert not m.is_stochastic() and m._resolve_keep(x, None) is i      # one draw for the step: the feature cache may hold
    assert m.is_stochastic()
    m.eval()
    assert not m.is_stochastic() and m.draw_keep_indices(2) is None and m._resolve_keep(x, None) is None     # eval(): all 1 + L tokens, the unchanged forward
    with pytest.raises(MfvitError, match="training-mode"):
        m._resolve_keep(x, i)
    m.train()
    m.patch_drop.prob = 0.0
    assert not m.is_stochastic() and m._resolve_keep(x, None) is None
    assert m._resolve_keep(x, torch.tensor([[3, 1], [0, 15]])).tolist() == [[3, 1], [0, 15]]         # explicit indices at rate 0
    for bad in ([[3, 16], [0, 1]], [[3, -1], [0, 1]], [[3, 3], [0, 1]], [[3, 1]]):
        with pytest.raises(MfvitError):
            m._resolve_keep(x, torch.tensor(bad))
    with pytest.raises(MfvitError):
        m._resolve_keep(x, torch.tensor([[0.0, 1.0], [2.0, 3.0]]))


def test_fus_crossvit_shares_one_draw_by_default():
    import importlib
    import vits
    fus = importlib.import_module("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
                                  "changemodelinputlocation_std002_sum")
    a, b = (vits.vit_small(depth=1, num_classes=3, patch_drop_rate=0.5, img_size=64) for _ in range(2))
    x = torch.zeros(2, 3, 64, 64)
    model = fus.Fus_CrossViT(a, b)
    assert model.patch_drop_shared is True
    ic, ie = model._draw_patch_keep(a, b, x, x)
    assert ic is ie and ic.shape == (2, 8)
    per = fus.Fus_CrossViT(a, b, patch_drop_shared=False)
    ic, ie = per._draw_patch_keep(a, b, x, x)
    assert ic.shape == ie.shape == (2, 8) and not torch.equal(ic, ie)
    b.patch_drop.prob = 0.75
    with pytest.raises(MfvitError, match="patch_drop_shared"):
        model._draw_patch_keep(a, b, x, x)
    a.eval(), b.eval()
    assert model._draw_patch_keep(a, b, x, x) == (None, None)


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mfvit.h")).read()
    lib = _lib.lib()
    assert lib.mfvit_abi_version() == 5 and _lib.ABI_VERSION == 5
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert "PatchDropout" in header
    assert ctypes.sizeof(_lib.VitCfg) == 21 * 4 and ctypes.sizeof(_lib.VitDrop) == 24       # the ABI-5 structs keep their layout


def vit_cfg(**kw):
    c = _lib.VitCfg()
    c.dtype, c.batch, c.img_h, c.img_w, c.dim, c.depth, c.heads, c.mlp_dim = _lib.BF16X3, 2, 224, 224, 384, 2, 12, 1536
    c.save_for_backward, c.ln_eps = 1, 1e-6
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_given_x0_entry_points_refuse_outside_their_domain():
    """Size query 0 and MFVIT_EINVAL before any HIP call (this test runs without a GPU): tokens out of range, a token-input cfg, the fp32 limit
    on the attention kernels' LDS, a NULL pointer."""
    lib = _lib.lib()
    size = lib.mfvit_vit_workspace_bytes_x0
    full = lib.mfvit_vit_workspace_bytes(vit_cfg())
    assert 0 < size(vit_cfg(), None, 2) < size(vit_cfg(), None, 99) < size(vit_cfg(), None, 197)
    assert size(vit_cfg(), None, 197) < full           # (no im2col buffer: the front end owns it)
    for t in (-1, 0, 1, 198, 1 << 30):
        assert size(vit_cfg(), None, t) == 0
    assert size(vit_cfg(token_input=1, tokens=64), None, 32) == 0
    assert size(vit_cfg(dtype=_lib.F32, img_h=512, img_w=512, heads=6), None, 99) == 0       # head_dim 64, T = 1025: refused for the full grid
    assert size(vit_cfg(dtype=_lib.F32), None, 99) > 0                                     # fp32 allows patch dropout
    assert size(vit_cfg(img_h=100), None, 9) == 0 and size(None, None, 9) == 0
    rates = (ctypes.c_float * 2)(0.0, 0.5)
    drop = _lib.VitDrop(0.0, 0.0, ctypes.cast(rates, ctypes.POINTER(ctypes.c_float)), 7)
    assert size(vit_cfg(), drop, 99) > size(vit_cfg(), None, 99)                            # a masked branch keeps a scratch row block
    assert size(vit_cfg(dtype=_lib.F32), drop, 99) == 0
    buf = ctypes.create_string_buffer(64)
    q = ctypes.addressof(buf)
    fwd, bwd = lib.mfvit_vit_forward_x0, lib.mfvit_vit_backward_x0
    for t in (1, 198):
        assert fwd(vit_cfg(), None, t, q, q, q, q, q, None) == -22
        assert bwd(vit_cfg(), None, t, q, q, q, q, q, q, 2, -1, None) == -22
    assert fwd(vit_cfg(token_input=1, tokens=64), None, 32, q, q, q, q, q, None) == -22
    for hole in range(5):
        a = [q] * 5
        a[hole] = None
        assert fwd(vit_cfg(), None, 99, *a, None) == -22, hole
    assert bwd(vit_cfg(), None, 99, None, q, q, q, q, q, 2, -1, None) == -22
    assert bwd(vit_cfg(), None, 99, q, None, q, q, q, q, 2, -1, None) == -22
    assert bwd(vit_cfg(), None, 99, q, q, None, q, q, q, 2, -1, None) == -22
    assert bwd(vit_cfg(), None, 99, q, q, q, None, q, q, 2, -1, None) == -22       # the final norm's stage needs dfeatures
    assert bwd(vit_cfg(), None, 99, q, q, q, q, q, None, 2, -1, None) == -22       # dx0 is required
    assert bwd(vit_cfg(), None, 99, q, q, q, q, q, q, 3, -1, None) == -22 and bwd(vit_cfg(), None, 99, q, q, q, q, q, q, 1, 2, None) == -22
    assert bwd(vit_cfg(save_for_backward=0), None, 99, q, q, q, q, q, q, 2, -1, None) == -22


def test_front_end_entry_points_refuse_outside_their_domain():
    lib = _lib.lib()
    size = lib.mfvit_patch_keep_workspace_bytes

    def pk(dtype=_lib.BF16X3, batch=2, h=224, w=224, keep=98, dim=384):
        return _lib.PatchKeepCfg(dtype, batch, h, w, keep, dim)
    assert 0 < size(pk(), 0) < size(pk(), 1)
    for bad in (pk(dtype=9), pk(batch=0), pk(h=100), pk(w=0), pk(keep=0), pk(keep=197), pk(dim=512), pk(batch=30000, keep=196)):
        assert size(bad, 1) == 0
    assert size(None, 1) == 0 and size(pk(h=96, w=64, keep=24), 1) > 0 and size(pk(h=96, w=64, keep=25), 1) == 0
    buf = ctypes.create_string_buffer(64)
    q = ctypes.addressof(buf)
    emb, bwd = lib.mfvit_patch_keep_embed, lib.mfvit_patch_keep_embed_bwd
    assert emb(pk(keep=0), q, q, q, q, q, q, q, 1, q, q, None) == -22
    for hole in (0, 1, 2, 3, 4, 5, 6, 8, 9):
        a = [q, q, q, q, q, q, q, 1, q, q]
        a[hole] = None
        assert emb(pk(), *a, None) == -22, hole
    assert bwd(pk(keep=197), q, q, q, q, q, q, q, q, None) == -22
    for hole in (0, 1, 2, 7):
        a = [q] * 8
        a[hole] = None
        assert bwd(pk(), *a, None) == -22, hole
    assert bwd(pk(), q, q, q, None, None, None, None, q, None) == -22              # nothing asked for
