"""CPU checks of attention-guided token pruning between blocks: the float64 restatement tests/token_prune_ref.py pinned against the unchanged
oracle, an independent plain-torch version and autograd; the conditions under which the GPU tests may demand the float64 selection (the float32
restatement selects the same sets, and the K-th and (K+1)-th scores lie at least 1e-3 apart); the host logic; wrong variants of the restatement
that the GPU gates must catch; and the C ABI's refusals, which load the library without a GPU."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import token_prune_ref as R
from mfvit import _lib
from mfvit._lib import MfvitError
from oracle import ref_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mfvit_vit_workspace_bytes_seg", "mfvit_vit_attn_layout_seg", "mfvit_vit_forward_seg", "mfvit_vit_backward_seg",
               "mfvit_token_score", "mfvit_token_select", "mfvit_token_reorg_fwd", "mfvit_token_reorg_bwd"]
WIDEST_F, WIDEST_G = max(f for f, _ in R.CAPS.values()), max(g for _, g in R.CAPS.values())
# The relative gap between the K-th and (K+1)-th float64 score, smallest over the images of each (case, stage), as score_gaps measures it on the
# seeds of token_prune_ref.CASES (patch dropout on / the same case in eval()); every one is at least 1e-3 = 50 x the 2e-5 forward error of bf16x3:
#   two_stage96  stage 0: 2.4e-03, stage 1: 1.7e-02      heads6_64   stage 0: 1.7e-02, stage 1: 4.8e-03      tile224      stage 0: 1.1e-03
#   base768      stage 0: 9.0e-03                        nofuse96    stage 0: 1.5e-02, stage 1: 3.1e-02      patchdrop96  stage 0: 4.2e-03 / eval 7.9e-03
MIN_GAP = 1e-3


# --------------------------------------------------------------------------------------------------- the restatement, pinned
def test_rate_one_is_the_oracle_encoder_exactly():
    for name in ("heads6_64", "nofuse96"):
        c = R.CASES[name]
        p = {k: v.double() for k, v in R.case_params(c).items()}
        img = R.rng(7101, (c["B"], 3) + c["hw"]).double()
        f, sel = R.features3d_pruned(p, img, c["blocks"], 1.0, c["fuse"], heads=c["heads"])
        assert sel == [] and torch.equal(f, ref_vit.features3d(p, img, c["heads"]))
        f, sel = R.features3d_pruned(p, img, (), 0.5, c["fuse"], heads=c["heads"])
        assert sel == [] and torch.equal(f, ref_vit.features3d(p, img, c["heads"]))


def plain_torch_stage(x, attn_cls, K, fuse):
    """An independent statement of one stage with torch.topk / torch.gather (valid on tie-free scores): x (B, T, D), attn_cls (B, h, T)."""
    s = attn_cls[:, :, 1:].mean(dim=1)
    top = torch.topk(s, K, dim=1).indices.sort(dim=1).values
    B, T, D = x.shape
    kept = torch.gather(x[:, 1:], 1, top[:, :, None].expand(-1, -1, D))
    out = [x[:, :1], kept]
    if fuse:
        mask = torch.ones(B, T - 1, dtype=torch.bool).scatter_(1, top, False)
        w = torch.where(mask, s, torch.zeros_like(s))
        w = w / w.sum(dim=1, keepdim=True)
        out.append(torch.einsum("bt,btd->bd", w, x[:, 1:])[:, None])
    return torch.cat(out, dim=1), top


@pytest.mark.parametrize("fuse", [True, False])
def test_restatement_against_plain_torch(fuse):
    g = torch.Generator().manual_seed(7)
    B, T, D, h, K = 3, 21, 16, 4, 9
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    a = torch.rand(B, h, T, generator=g, dtype=torch.float64)
    s = a[:, :, 1:].mean(dim=1)
    keep, drop = R.select(s, K)
    want, top = plain_torch_stage(x, a, K, fuse)
    assert torch.equal(keep, top)
    assert torch.allclose(R.reorg(x, s, keep, fuse), want, rtol=1e-13, atol=1e-13)
    org = R.token_origin([keep], T, fuse)
    assert torch.equal(org[:, :K], keep) and (not fuse or bool((org[:, K] == -1).all()))


def test_selection_order_ties_nan_and_the_uniform_fallback():
    s = np.array([[3, 1, 3, 3, 0, 1, 3, 2, 2, 3, 1, 0.0], [np.nan, 1, 2, np.nan, 3, 4] + [np.nan] * 6, [0.0] * 12], dtype=np.float32)
    keep, drop, w = R.select_ref(s, 5)
    assert keep.tolist() == [[0, 2, 3, 6, 9], [0, 1, 2, 4, 5], [0, 1, 2, 3, 4]]
    assert all(sorted(keep[b].tolist() + drop[b].tolist()) == list(range(12)) for b in range(3))
    assert np.allclose(w[0].sum(), 1.0) and (w[1] == np.float32(1 / 7)).all() and (w[2] == np.float32(1 / 7)).all()
    assert R.rank_ref(np.array([[0.0, -0.0, 1.0]])).tolist() == [[1, 2, 0]]          # -0.0 == +0.0: a tie, the lower index first
    # a single dropped row: weight exactly one, the fused row is that row
    x = R.rng(7102, (1, 13, 8)).numpy()
    keep, drop, w = R.select_ref(s[:1], 11)
    assert w.tolist() == [[1.0]] and np.array_equal(R.reorg_fwd_ref(x, keep, drop, w, 1)[0, -1], x[0, 1 + drop[0, 0]].astype(np.float64))


def test_stated_backward_is_the_gradient_of_the_restatement():
    """Autograd through the restatement's stage (constant selection and weights) equals the stated backward: cls and kept rows of dx' copied,
    w_j dx'[fused] on every dropped row (exact zeros without a fused row)."""
    g = torch.Generator().manual_seed(11)
    B, T, D, K = 2, 15, 8, 6
    for fuse in (True, False):
        x = torch.randn(B, T, D, generator=g, dtype=torch.float64, requires_grad=True)
        s = torch.rand(B, T - 1, generator=g, dtype=torch.float64)
        keep, drop = R.select(s, K)
        out = R.reorg(x, s, keep, fuse)
        dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
        (out * dout).sum().backward()
        want = torch.zeros(B, T, D, dtype=torch.float64)
        want[:, 0] = dout[:, 0]
        w = R.weights(s, drop)
        for b in range(B):
            want[b, 1 + keep[b]] = dout[b, 1:1 + K]
            if fuse:
                want[b, 1 + drop[b]] = w[b][:, None] * dout[b, 1 + K][None]
        assert torch.allclose(x.grad, want, rtol=1e-14, atol=1e-14)
        if not fuse:
            assert bool((x.grad[0, 1 + drop[0]] == 0).all())
        # the f32 kernel reference states the same thing
        got = R.reorg_bwd_ref(dout.float().numpy(), keep.numpy(), drop.numpy(), w.float().numpy(), T, int(fuse))
        assert np.allclose(got, want.numpy(), rtol=1e-5, atol=1e-6)


# --------------------------------------------------------------------------------------------------- the conditions of the selection demand
@pytest.mark.parametrize("name,patch", [(n, True) for n in R.CASES] + [(n, False) for n, c in R.CASES.items() if c["patch_keep"]])
def test_float32_restatement_selects_the_float64_sets_and_the_gaps_hold(name, patch):
    """patch=False: a case with patch dropout in front once more without it - what the model runs in eval()."""
    ref = R.reference(name, patch)
    got = R.run(name, torch.float32, grads=False, patch=patch)
    assert len(ref["indices"]) == len(got["indices"]) > 0
    assert all(torch.equal(a, b) for a, b in zip(ref["indices"], got["indices"]))
    assert R.scale_err(got["features"], ref["features"]) < R.CAPS["fp32"][0] / 10
    gaps = R.score_gaps(name, patch)
    assert len(gaps) == len(ref["indices"]) * R.CASES[name]["B"]
    assert min(g for _, _, g in gaps) >= MIN_GAP, gaps


# --------------------------------------------------------------------------------------------------- host logic
def test_token_schedule_and_the_skip():
    import vits
    m = vits.vit_small(num_classes=3, token_keep_rate=0.7)
    assert m.token_prune_blocks == (3, 6, 9) and m.token_fuse is True
    assert m.token_schedule() == [197, 140, 100, 72] == R.token_schedule(197, 12, (3, 6, 9), 0.7, True)
    assert m._token_segments(197) == [(0, 4, 197), (4, 7, 140), (7, 10, 100), (10, 12, 72)]
    m.token_fuse = False
    assert m.token_schedule() == [197, 139, 98, 69]
    m.token_fuse, m.token_keep_rate = True, 0.5
    assert m.token_schedule() == [197, 100, 52, 28] and m.token_schedule(99) == [99, 51, 27, 15]
    m.token_keep_rate = 1.0
    assert m.token_schedule() == [197] and not m.token_pruning_active()
    assert vits.vit_base(num_classes=3, depth=8).token_prune_blocks == (2, 4, 6)
    assert vits.vit_small(num_classes=3, depth=2).token_prune_blocks == (0,) and vits.vit_small(num_classes=3, depth=1).token_prune_blocks == ()
    assert not vits.vit_small(num_classes=3).token_pruning_active()                  # the default rate is 1.0
    # K == T - 1: the stage is skipped, the sequence and the segment go on
    s = vits.vit_small(num_classes=3, depth=4, img_size=64, token_keep_rate=0.97, token_prune_blocks=(0, 1, 2))
    assert [R.num_keep(T, 0.97) for T in (17, 5, 3)] == [16, 4, 2]
    assert s.token_schedule() == [17] and s._token_segments(17) == [(0, 4, 17)]
    s.token_keep_rate = 0.9                          # ceil(0.9 * 16) = 15 < 16: one row goes, and with the fused row the count stays 17
    assert s.token_schedule() == [17, 17, 17, 17]
    assert R.num_keep(197, 0.7) == math.ceil(0.7 * 196) == 138 and R.num_keep(2, 0.01) == 1
    assert list(m.state_dict()) == list(vits.vit_small(num_classes=3).state_dict())


def test_argument_refusals():
    import vits
    for kw in (dict(token_keep_rate=0.0), dict(token_keep_rate=1.5), dict(token_keep_rate=float("nan")), dict(token_prune_blocks=(3, 3)),
               dict(token_prune_blocks=(6, 3)), dict(token_prune_blocks=(11,)), dict(token_prune_blocks=(-1,)), dict(token_prune_blocks=(1.5,))):
        with pytest.raises(MfvitError):
            vits.vit_small(num_classes=3, **kw)
    m = vits.vit_small(num_classes=3, depth=3, img_size=64, token_keep_rate=0.5, token_prune_blocks=(0, 1))
    assert m.token_schedule() == [17, 10, 7]
    for bad in (1, 18):
        with pytest.raises(MfvitError):
            m.token_schedule(bad)
    with pytest.raises(MfvitError):
        m.token_origin()                            # no pruned forward has run
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(MfvitError):                 # valid arguments, CPU tensor: loud failure, no fallback
        m.features3D(x)
    good = [torch.arange(8).expand(2, 8), torch.arange(4).expand(2, 4)]
    for bad in ([good[0]], [good[0][:, :7], good[1]], [good[0].float(), good[1]], [good[0] + 9, good[1]], [good[0] * 0, good[1]], good[0]):
        with pytest.raises(MfvitError):
            m._check_token_indices(bad, 2, 17)
    m.token_keep_rate = 1.0
    with pytest.raises(MfvitError, match="token_indices"):
        m.features3D(x, token_indices=good)
    m.token_keep_rate = 2.0                          # a plain attribute: checked when it is used
    with pytest.raises(MfvitError):
        m.token_schedule()


def test_fus_crossvit_refuses_encoders_that_prune_differently():
    import vits
    fus = importlib.import_module("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
                                  "changemodelinputlocation_std002_sum")
    mk = lambda **kw: vits.vit_small(depth=3, num_classes=3, img_size=64, **kw)      # noqa: E731
    a = mk(token_keep_rate=0.5, token_prune_blocks=(0,))
    check = fus.Fus_CrossViT._check_token_pruning
    check(a, mk(token_keep_rate=0.5, token_prune_blocks=(0,)))
    check(mk(), mk(token_keep_rate=1.0, token_prune_blocks=(1,)))                      # nothing is pruned: nothing to compare
    for other, word in ((mk(token_keep_rate=0.7, token_prune_blocks=(0,)), "token_keep_rate"), (mk(), "one encoder"),
                        (mk(token_keep_rate=0.5, token_prune_blocks=(0, 1)), "token_prune_blocks"),
                        (mk(token_keep_rate=0.5, token_prune_blocks=(0,), token_fuse=False), "token_fuse"),
                        (vits.vit_small(depth=3, num_classes=3, img_size=96, token_keep_rate=0.5, token_prune_blocks=(0,)), "token grid")):
        with pytest.raises(MfvitError, match=word):
            check(a, other)


# --------------------------------------------------------------------------------------------------- wrong variants against the GPU gates
@pytest.mark.parametrize("mutation", list(R.MUTATIONS))
def test_wrong_restatements_fail_the_gates(mutation):
    """Each wrong variant, in float64 on the GPU tests' own inputs, misses what tests/test_token_prune_gpu.py asserts in EVERY precision: the
    output shape, or the widest feature / gradient gate of CAPS."""
    name = "heads6_64" if mutation == "floor_K" else "two_stage96"
    ref = R.reference(name)
    if mutation == "floor_K":                       # 0.7 * 16 = 11.2: floor keeps 11 rows where ceil keeps 12 - the output shape the GPU test asserts
        got = R.run(name, torch.float64, grads=False, **R.MUTATIONS[mutation])
        assert got["features"].shape[1] < ref["features"].shape[1] and got["indices"][0].shape[1] == 11
        return
    got = R.run(name, torch.float64, indices=ref["indices"], **R.MUTATIONS[mutation])
    e_f = R.scale_err(got["features"], ref["features"])
    e_g = max(max(R.scale_err(got["grads"][k], g) for k, g in ref["grads"].items()), R.scale_err(got["dimg"], ref["dimg"]))
    print(f"{mutation}: features {e_f:.2e} gradients {e_g:.2e}")
    assert e_f > WIDEST_F or e_g > WIDEST_G, (e_f, e_g)
    if mutation != "fused_grad_not_distributed":
        assert e_f > WIDEST_F, e_f


# --------------------------------------------------------------------------------------------------- the C ABI without a GPU
def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mfvit.h")).read()
    lib = _lib.lib()
    assert lib.mfvit_abi_version() == 5 and _lib.ABI_VERSION == 5
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert ctypes.sizeof(_lib.VitSeg) == 16 and ctypes.sizeof(_lib.VitCfg) == 21 * 4


def vit_cfg(**kw):
    c = _lib.VitCfg()
    c.dtype, c.batch, c.img_h, c.img_w, c.dim, c.depth, c.heads, c.mlp_dim = _lib.BF16X3, 2, 224, 224, 384, 4, 12, 1536
    c.save_for_backward, c.ln_eps = 1, 1e-6
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_block_range_entry_points_refuse_outside_their_domain():
    """Size query 0 and MFVIT_EINVAL before any HIP call (this test runs without a GPU)."""
    lib = _lib.lib()
    size, seg = lib.mfvit_vit_workspace_bytes_seg, _lib.VitSeg
    full = seg(0, 4, 197, 1)
    assert size(vit_cfg(), None, full, 0) == lib.mfvit_vit_workspace_bytes(vit_cfg())
    assert size(vit_cfg(), None, full, 1) == lib.mfvit_vit_workspace_bytes_ex(vit_cfg(), None, 1)
    assert size(vit_cfg(), None, seg(0, 4, 99, 0), 0) == lib.mfvit_vit_workspace_bytes_x0(vit_cfg(), None, 99)
    assert 0 < size(vit_cfg(), None, seg(1, 2, 99, 0), 0) < size(vit_cfg(), None, seg(1, 3, 99, 0), 0) < size(vit_cfg(), None, seg(0, 4, 99, 0), 0)
    bad = [seg(-1, 2, 99, 0), seg(2, 2, 99, 0), seg(3, 2, 99, 0), seg(0, 5, 99, 0), seg(1, 2, 1, 0), seg(1, 2, 198, 0), seg(1, 2, 99, 2),
           seg(1, 2, 99, -1), seg(1, 2, 197, 1), seg(0, 2, 99, 1)]
    for s in bad:
        assert size(vit_cfg(), None, s, 0) == 0, (s.block_lo, s.block_hi, s.tokens, s.image_in)
    assert size(vit_cfg(), None, None, 0) == 0 and size(None, None, full, 0) == 0
    assert size(vit_cfg(token_input=1, tokens=64), None, seg(0, 2, 32, 0), 0) == 0
    assert size(vit_cfg(img_h=100), None, full, 0) == 0
    assert size(vit_cfg(), None, seg(1, 2, 99, 0), 1) == 0 and size(vit_cfg(save_for_backward=0), None, full, 1) == 0      # want_dimg
    assert size(vit_cfg(dtype=_lib.F32, img_h=512, img_w=512, heads=6), None, seg(0, 2, 99, 0), 0) == 0
    out = (ctypes.c_int64 * 4)()
    lay = lib.mfvit_vit_attn_layout_seg
    assert lay(vit_cfg(), None, seg(1, 3, 99, 0), out) == 0 and out[0] > 0 and out[1] > out[0] and out[2] > 0 and out[3] == _lib.X3F16
    assert lay(vit_cfg(save_for_backward=0), None, seg(1, 3, 99, 0), out) == 0 and out[2] == 0
    assert lay(vit_cfg(), None, bad[0], out) == -22 and lay(vit_cfg(), None, full, None) == -22 and lay(vit_cfg(), None, None, out) == -22
    buf = ctypes.create_string_buffer(64)
    q = ctypes.addressof(buf)
    fwd, bwd = lib.mfvit_vit_forward_seg, lib.mfvit_vit_backward_seg
    mid = seg(1, 3, 99, 0)
    for s in bad + [None]:
        assert fwd(vit_cfg(), None, s, q, q, q, q, q, None) == -22
        assert bwd(vit_cfg(), None, s, q, q, q, q, q, q, None, 2, 1, None) == -22
    for hole in range(5):
        a = [q] * 5
        a[hole] = None
        assert fwd(vit_cfg(), None, mid, *a, None) == -22, hole
    for hole in (0, 1, 2, 3, 5):                    # params, shadow, workspace, dx_out (the entry stage needs it), dx_in
        a = [q] * 6
        a[hole] = None
        assert bwd(vit_cfg(), None, mid, *a, None, 3, 0, None) == -22, hole
    for hi, lo in ((4, 0), (3, -1), (1, 2), (0, -1)):
        assert bwd(vit_cfg(), None, mid, q, q, q, q, q, q, None, hi, lo, None) == -22, (hi, lo)
    assert bwd(vit_cfg(), None, mid, q, q, q, q, q, q, q, 3, 0, None) == -22                       # d img belongs to the range that takes the image
    assert bwd(vit_cfg(), None, full, q, q, q, q, None, None, None, 4, -1, None) == -22            # no parameter gradient and no d img
    assert bwd(vit_cfg(), None, full, q, q, q, q, q, None, q, 4, 0, None) == -22                   # d img without the embedding stage
    assert bwd(vit_cfg(save_for_backward=0), None, mid, q, q, q, q, q, q, None, 3, 0, None) == -22
    assert fwd(vit_cfg(token_input=1, tokens=64), None, seg(0, 2, 32, 0), q, q, q, q, q, None) == -22


def test_token_kernels_refuse_outside_their_domain():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    q = (ctypes.addressof(buf) + 15) & ~15
    score, select, fwd, bwd = lib.mfvit_token_score, lib.mfvit_token_select, lib.mfvit_token_reorg_fwd, lib.mfvit_token_reorg_bwd
    for a in ((9, q, q, 2, 17, 12, 32, q, q), (-1, q, q, 2, 17, 12, 32, q, q), (0, None, q, 2, 17, 12, 32, q, q), (0, q, None, 2, 17, 12, 32, q, q),
              (0, q, q, 0, 17, 12, 32, q, q), (0, q, q, 70000, 17, 12, 32, q, q), (0, q, q, 2, 1, 12, 32, q, q), (0, q, q, 2, 8194, 12, 32, q, q),
              (0, q, q, 2, 17, 0, 32, q, q), (0, q, q, 2, 17, 12, 48, q, q), (0, q, q, 2, 17, 12, 32, None, q), (0, q, q, 2, 17, 12, 32, q, None)):
        assert score(*a, None) == -22, a
    for a in ((None, 16, 2, 16, 8, None, q, q, q, q), (q, 16, 2, 16, 8, None, None, q, q, q), (q, 16, 2, 16, 8, None, q, None, q, q),
              (q, 16, 2, 16, 8, None, q, q, None, q), (q, 15, 2, 16, 8, None, q, q, q, q), (q, 16, 0, 16, 8, None, q, q, q, q),
              (q, 16, 70000, 16, 8, None, q, q, q, q), (q, 16, 2, 0, 8, None, q, q, q, q), (q, 8193, 2, 8193, 8, None, q, q, q, q),
              (q, 16, 2, 16, 0, None, q, q, q, q), (q, 16, 2, 16, 17, None, q, q, q, q), (q, 16, 2, 16, 8, q, q, q, q, None)):
        assert select(*a, None) == -22, a
    q2 = q + 128
    for f in (fwd, bwd):
        for a in ((None, q, q, q, q2, 2, 17, 384, 8, 1, q), (q, None, q, q, q2, 2, 17, 384, 8, 1, q), (q, q, None, q, q2, 2, 17, 384, 8, 1, q),
                  (q, q, q, None, q2, 2, 17, 384, 8, 1, q), (q, q, q, q, None, 2, 17, 384, 8, 1, q), (q, q, q, q, q2, 2, 17, 384, 8, 1, None),
                  (q + 4, q, q, q, q2, 2, 17, 384, 8, 1, q), (q, q, q, q, q2 + 8, 2, 17, 384, 8, 1, q), (q, q, q, q, q, 2, 17, 384, 8, 1, q),
                  (q, q, q, q, q2, 0, 17, 384, 8, 1, q), (q, q, q, q, q2, 70000, 17, 384, 8, 1, q), (q, q, q, q, q2, 2, 1, 384, 8, 1, q),
                  (q, q, q, q, q2, 2, 8194, 384, 8, 1, q), (q, q, q, q, q2, 2, 17, 512, 8, 1, q), (q, q, q, q, q2, 2, 17, 384, 0, 1, q),
                  (q, q, q, q, q2, 2, 17, 384, 17, 1, q), (q, q, q, q, q2, 2, 17, 384, 16, 1, q), (q, q, q, q, q2, 2, 17, 384, 8, 2, q),
                  (q, q, q, q, q2, 30000, 197, 768, 8, 1, q)):
            assert f(*a, None) == -22, a
