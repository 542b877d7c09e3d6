"""The ViT encoder's one forward / backward chain (mfvit/encoder.py): what the host decides before anything is launched, no GPU needed.

The Python side runs every forward as a list of block ranges through mfvit_vit_forward_seg / _backward_seg; the range [0, depth) stands for the
whole-stack entry points (include/mfvit.h), so its workspace must have their size."""
import ctypes

import pytest


def _lib():
    from mfvit import _lib
    return _lib


def _cfg(dtype, dim, save=1, depth=2, hw=64):
    L = _lib()
    c = L.VitCfg()
    c.dtype = L.dtype_code(dtype)
    c.batch, c.img_h, c.img_w = 2, hw, hw
    c.dim, c.depth, c.heads, c.mlp_dim = dim, depth, dim // 64, 4 * dim
    c.save_for_backward = save
    c.ln_eps = 1e-6
    return c


def _drop(depth=2):
    L = _lib()
    r = (ctypes.c_float * depth)(*[0.2 * l / max(1, depth - 1) for l in range(depth)])
    d = L.VitDrop(0.1, 0.1, ctypes.cast(r, ctypes.POINTER(ctypes.c_float)), 7)
    d._r = r
    return d


@pytest.mark.parametrize("dim", [384, 768])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3", "fp16"])
@pytest.mark.parametrize("with_drop", [False, True])
def test_the_full_range_has_the_workspace_of_the_whole_stack(dtype, dim, with_drop):
    L = _lib()
    h = L.lib()
    cfg = _cfg(dtype, dim)
    drop = _drop() if with_drop else None
    T = (cfg.img_h // 16) * (cfg.img_w // 16) + 1
    valid = not (with_drop and dtype == "fp32")            # (the dropout stages exist for the 16-bit operand types: both queries answer 0)
    for w in (0, 1):
        whole = h.mfvit_vit_workspace_bytes_ex(cfg, drop, w)
        assert (whole > 0) == valid
        assert h.mfvit_vit_workspace_bytes_seg(cfg, drop, L.VitSeg(0, cfg.depth, T, 1), w) == whole
    for t in (2, 9, T):
        x0 = h.mfvit_vit_workspace_bytes_x0(cfg, drop, t)
        assert (x0 > 0) == valid
        assert h.mfvit_vit_workspace_bytes_seg(cfg, drop, L.VitSeg(0, cfg.depth, t, 0), 0) == x0
    # the plain size queries are the _ex one without the image gradient
    assert h.mfvit_vit_workspace_bytes_ex(cfg, drop, 0) == (h.mfvit_vit_workspace_bytes_drop(cfg, drop) if with_drop else h.mfvit_vit_workspace_bytes(cfg))


# --------------------------------------------------------------------------------------------------- the backward's call list
# VisionTransformerMoCo._backward_calls turns (block ranges, stage groups) into the mfvit_vit_backward_seg calls of one backward:
# per group [(range index, stage_hi, stage_lo, then)], then in {"reorg", "front", None}.  Depth 12 throughout.
DEPTH = 12
GROUPS = {      # _grad_bucket_layers (None: no stage hook) -> the (hi, lo) groups of _stage_groups
    None: [(12, -1)],
    1: [(12, 11), (10, 10), (9, 9), (8, 8), (7, 7), (6, 6), (5, 5), (4, 4), (3, 3), (2, 2), (1, 1), (0, -1)],
    4: [(12, 8), (7, 4), (3, -1)],
    12: [(12, -1)],
}
THREE = [(0, 4), (4, 7), (7, 12)]
# the calls the two-driver code made for THREE (recorded once from its backward with a stub library); `X`: what follows the call that reaches
# stage -1 - nothing, or the front end's backward.  With 4 blocks per group the edge 4 | 3 is the boundary of ranges 0 and 1, the edge 8 | 7
# falls inside range 2.
def _three(X):
    whole = [[(2, 12, 6, "reorg"), (1, 7, 3, "reorg"), (0, 4, -1, X)]]
    return {
        None: whole,
        1: [[(2, 12, 11, None)], [(2, 10, 10, None)], [(2, 9, 9, None)], [(2, 8, 8, None)], [(2, 7, 6, "reorg")], [(1, 7, 6, None)], [(1, 5, 5, None)],
            [(1, 4, 3, "reorg")], [(0, 4, 3, None)], [(0, 2, 2, None)], [(0, 1, 1, None)], [(0, 0, -1, X)]],
        4: [[(2, 12, 8, None)], [(2, 7, 6, "reorg"), (1, 7, 3, "reorg")], [(0, 4, -1, X)]],
        12: whole,
    }


def _calls(ranges, gb, front=False):
    from mfvit.encoder import VisionTransformerMoCo
    return VisionTransformerMoCo._backward_calls(ranges, GROUPS[gb], DEPTH, front)


@pytest.fixture(scope="module")
def model():
    import vits
    return vits.vit_small(num_classes=3, depth=DEPTH, img_size=64)


@pytest.mark.parametrize("gb", [None, 1, 4, 12])
def test_stage_groups(model, gb):
    model._grad_bucket_layers = gb or 4
    assert model._stage_groups(gb is not None) == GROUPS[gb]


@pytest.mark.parametrize("gb", [None, 1, 4, 12])
@pytest.mark.parametrize("front", [False, True])
def test_one_range_runs_the_stage_groups_verbatim(gb, front):
    """the full grid (front = False: the image goes in, d img may ride with the call whose stage_lo is -1) and a patch-dropout sequence (front =
    True: the front end's backward follows that call, and no other)"""
    calls = _calls([(0, DEPTH)], gb, front)
    assert [[(hi, lo) for _, hi, lo, _ in g] for g in calls] == [[g] for g in GROUPS[gb]]
    flat = [c for g in calls for c in g]
    assert all(i == 0 for i, _, _, _ in flat)
    assert [then for _, _, lo, then in flat if lo == -1] == (["front"] if front else [None])        # (one call reaches the embedding stage)
    assert all(then is None for _, _, lo, then in flat if lo != -1)


@pytest.mark.parametrize("gb", [None, 1, 4, 12])
@pytest.mark.parametrize("front", [False, True])
def test_three_ranges_give_the_recorded_calls(gb, front):
    assert _calls(THREE, gb, front) == _three("front" if front else None)[gb]


@pytest.mark.parametrize("gb", [None, 1, 4, 12])
def test_three_ranges_cover_every_stage_once(gb):
    calls = _calls(THREE, gb)
    assert len(calls) == len(GROUPS[gb])
    flat = [c for g in calls for c in g]
    stages = []
    for i, hi, lo, _ in flat:
        a, b = THREE[i]
        assert a - 1 <= lo <= hi <= b
        if hi == b == DEPTH:
            stages.append(DEPTH)                                    # the final norm
        stages += range(min(hi, b - 1), max(lo, a) - 1, -1)         # the blocks
        if lo == -1:
            stages.append(-1)                                       # the embedding
    assert stages == list(range(DEPTH, -2, -1))                     # every model stage once, descending
    for (hi_g, lo_g), g in zip(GROUPS[gb], calls):                  # a group's calls stay inside its model stages
        for i, hi, lo, _ in g:
            a, b = THREE[i]
            assert lo_g <= max(lo, a) and min(hi, b - 1) <= hi_g
    for r, (a, b) in enumerate(THREE):
        mine = [(hi, lo, then) for i, hi, lo, then in flat if i == r]
        assert [hi >= b - 1 >= lo for hi, lo, _ in mine if hi == b] == [True]         # the entry stage rides with the top block
        assert [hi >= a >= lo for hi, lo, _ in mine if lo == a - 1] == [True]         # block_lo - 1 rides with the bottom block
        # the reorganisation's backward follows exactly the call that reaches block_lo - 1 of ranges 1 and 2
        assert [then for hi, lo, then in mine] == [("reorg" if r > 0 else None) if lo == a - 1 else None for hi, lo, _ in mine]
