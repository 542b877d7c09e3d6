"""Per-head attention statistics without a GPU: the float64 restatement of tests/attn_stats_ref.py pinned to an independent form, the f32 floor
under its gate, the mutations the gate must catch, the C ABI's host-side behaviour (symbols, workspace layout, EINVAL domain) and the head
spread that makes the end-to-end GPU test meaningful."""
import ctypes
import re

import numpy as np
import pytest
import torch

import attn_stats_ref as R
from conftest import ROOT, rng_tensor

EINVAL, ENOSYS = -22, -38


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("gh,gw", [(1, 1), (2, 2), (3, 5), (14, 14)])
def test_restatement_equals_an_independent_einsum_form(gh, gw):
    T, patch = gh * gw + 1, 16.0
    P = torch.from_numpy(R.probs_from_qk(R.gaussian_qk(3, 2, T, 3, 8)))
    i = torch.arange(T - 1)
    yx = torch.stack([i // gw, i % gw], dim=1).double()
    d = patch * torch.cdist(yx, yx)
    Pp = P[..., 1:, 1:]
    want = torch.stack([
        torch.einsum("bhij,ij->bh", Pp, d) / (T - 1),
        (torch.einsum("bhij,ij->bhi", Pp, d) / Pp.sum(-1)).mean(-1),
        torch.special.entr(P).sum(-1).mean(-1),
        torch.special.entr(P[..., 0, :]).sum(-1),
        P[..., 1:, 0].mean(-1),
        torch.diagonal(P, dim1=-2, dim2=-1).mean(-1)], dim=-1).numpy()
    got = R.stats(P.numpy(), gh, gw, patch)
    assert got.shape == (2, 3, 6)
    assert np.abs(got - want).max() <= 1e-12 * (np.abs(want).max() + patch)
    if T == 2:
        assert np.all(got[..., :2] == 0)                             # one patch: both distances are 0


def test_gate_is_the_formula():
    ref = np.array([[100.0, 50.0, 3.0, 2.0, 0.01, 0.2]])
    g = R.gates(197, ref, 16.0)
    u = 2.0 ** -24
    assert np.allclose(g[0], [213 * u * 116, 2 * 213 * u * 66, 213 * u * 4, 213 * u * 3, 213 * u * 1.01, 213 * u * 1.2], rtol=1e-15)


# ------------------------------------------------------------------------------------------------ 2. the f32 floor
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_f32_floor_sits_under_a_quarter_of_the_gate(case):
    _, gh, gw, B, H, hd = case
    T = gh * gw + 1
    P = R.probs_from_qk(R.gaussian_qk(11, B, T, H, hd))
    ref = R.stats(P, gh, gw)
    share = float((np.abs(R.f32_floor(P, gh, gw) - ref) / R.gates(T, ref)).max())
    print(f"{R.case_id(case)}: f32 floor at {share:.3f} of the gate")
    assert share < 0.25


# ------------------------------------------------------------------------------------------------ 3. mutations
def test_gate_catches_the_mutations():
    gh, gw, H = 10, 20, 3
    T = gh * gw + 1
    P = R.probs_from_qk(R.gaussian_qk(12, 1, T, H, 64))
    ref = R.stats(P, gh, gw)
    g = R.gates(T, ref)

    def miss(mut):
        return float((np.abs(mut - ref) / g).max())
    dropped = P.copy()
    dropped[..., T - 1] = 0.0
    d = R.distances(gh, gw)
    cls_row = ref.copy()                                              # the cls row counted with the coordinates its clamped index gives it (patch 0's)
    cls_row[..., 0] += (P[..., 0, 1:] * d[1, 1:]).sum(-1) / (T - 1)
    found = {"last key dropped": miss(R.stats(dropped, gh, gw)), "cls row counted in distance": miss(cls_row),
             "heads rolled by one": miss(np.roll(ref, 1, axis=1)), "gw and gh swapped": miss(R.stats(P, gw, gh))}
    print(found)
    for name, m in found.items():
        assert m >= 10.0, (name, m)


# ------------------------------------------------------------------------------------------------ 4. symbols
NEW = {"mfvit_vit_attn_layout": 2, "mfvit_attention_stats_work_bytes": 4, "mfvit_attention_stats": 17}


def test_new_symbols_are_declared_exported_and_bound():
    from mfvit import _lib, attnstats
    h = _lib.lib()
    header = open(f"{ROOT}/include/mfvit.h").read()
    for name, arity in NEW.items():
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(h, name), name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    assert int(re.search(r"#define MFVIT_ATTN_NSTAT (\d+)", header).group(1)) == len(attnstats.STATS) == 6
    assert attnstats.STATS == R.STATS
    assert h.mfvit_abi_version() == 5 and _lib.ABI_VERSION == 5


# ------------------------------------------------------------------------------------------------ 5. the workspace layout
@pytest.mark.parametrize("img", [224, 384])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16", "bf16x3"])
def test_attn_layout_lies_inside_the_workspace(precision, img):
    import vits
    from mfvit import _lib
    h = _lib.lib()
    depth, B = 3, 2
    m = vits.vit_small(num_classes=3, depth=depth, img_size=img, precision=precision)
    x = torch.zeros(B, 3, img, img)
    cfg = m._cfg(x, True)
    out = (ctypes.c_int64 * 4)()
    assert h.mfvit_vit_attn_layout(cfg, out) == 0
    T, H, hd = m.num_tokens, m.num_heads, m.embed_dim // m.num_heads
    tag = h.mfvit_attention_qkv_dtype(_lib.dtype_code(precision), T, hd)
    assert out[3] == tag
    es = {_lib.F32: 4, _lib.BF16: 2, _lib.F16: 2, _lib.BF16X3: 4, _lib.X3F16: 4}[tag]
    qkv_bytes, lse_bytes = B * T * 3 * m.embed_dim * es, B * H * T * 4
    total = h.mfvit_vit_workspace_bytes(cfg)
    assert all(o >= 0 and o % 16 == 0 for o in out[:3])
    assert out[2] >= qkv_bytes + lse_bytes
    assert out[0] + qkv_bytes <= out[1] or out[1] + lse_bytes <= out[0]         # the two do not overlap
    assert out[0] + (depth - 1) * out[2] + qkv_bytes <= total and out[1] + (depth - 1) * out[2] + lse_bytes <= total
    assert out[0] + depth * out[2] <= total + out[2]
    assert h.mfvit_vit_attn_layout(m._cfg(x, False), out) == EINVAL             # nothing is kept without save_for_backward
    assert h.mfvit_vit_attn_layout(cfg, None) == EINVAL
    assert h.mfvit_vit_attn_layout(None, out) == EINVAL
    assert h.mfvit_vit_attn_layout(m._cfg(torch.zeros(B, 3, img, img - 4), True), out) == EINVAL
    tok = m._cfg(x, True)
    tok.token_input, tok.tokens = 1, T
    assert h.mfvit_vit_attn_layout(tok, out) == EINVAL                          # token-input mode


# ------------------------------------------------------------------------------------------------ 6. the EINVAL domain
def test_stats_einval_domain_needs_no_gpu():
    from mfvit import _lib
    h = _lib.lib()
    # (host addresses that are never dereferenced: every call below is refused before any HIP call)
    buf = (ctypes.c_double * 64)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    wb = h.mfvit_attention_stats_work_bytes(2, 3, 197, 12)
    assert wb == 2 * 3 * 12 * 7 * 6 * 8
    for bad in ((0, 3, 197, 12), (2, 0, 197, 12), (2, 3, 1, 12), (2, 3, 197, 0), (-1, 3, 197, 12), (4096, 4096, 577, 12)):
        assert h.mfvit_attention_stats_work_bytes(*bad) == 0, bad
    ok = dict(dt=_lib.F32, qkv=a, lse=a, qs=1024, ls=256, nblk=2, B=3, T=197, H=12, hd=32, gh=14, gw=14, stats=a, work=a, wb=wb)

    def call(**kw):
        c = dict(ok, **kw)
        return h.mfvit_attention_stats(c["dt"], c["qkv"], c["lse"], c["qs"], c["ls"], c["nblk"], c["B"], c["T"], c["H"], c["hd"], c["gh"], c["gw"],
                                       16.0, c["stats"], c["work"], c["wb"], None)
    for bad in (dict(qkv=None), dict(lse=None), dict(stats=None), dict(work=None), dict(nblk=0), dict(B=0), dict(H=0), dict(gh=0), dict(gw=0),
                dict(gh=-14, gw=-14), dict(T=196), dict(T=198), dict(gh=14, gw=13), dict(qs=1032), dict(ls=260), dict(qs=8), dict(wb=wb - 1),
                dict(wb=0), dict(nblk=4096, B=4096, T=577, gh=24, gw=24, wb=1 << 62), dict(dt=5), dict(dt=-1)):
        assert call(**bad) == EINVAL, bad
    for hd in (16, 48, 128, 0):
        assert call(hd=hd) == ENOSYS, hd


def test_python_surface():
    import vits
    from mfvit import _lib, attnstats
    m = vits.vit_small(num_classes=3, depth=2)
    assert callable(m.attention_stats)
    with pytest.raises(_lib.MfvitError):
        m.attention_stats(torch.zeros(1, 3, 224, 224))                          # no eager fallback
    with pytest.raises(_lib.MfvitError):
        attnstats.attention_stats(torch.zeros(8), torch.zeros(8), _lib.F32, 1, 2, 1, 32, (1, 1))
    with pytest.raises(ValueError):
        m.attention_stats(torch.zeros(1, 3, 224, 224), blocks=[2])
    with pytest.raises(ValueError):
        attnstats.AttentionStatsMeter(0, 12)
    with pytest.raises(RuntimeError):
        attnstats.AttentionStatsMeter(2, 12).result()


# ------------------------------------------------------------------------------------------------ 7. distinct heads for the end-to-end test
def test_x4_weights_make_the_heads_distinct():
    from oracle import ref_vit
    from test_attention_maps_gpu import ref_probs
    sd = R.x4_params(ref_vit.seeded_params(7, arch="vit_small", num_classes=3, depth=2))
    import vits
    sd["pos_embed"] = vits.vit_small(num_classes=3, depth=2).pos_embed.detach().clone()
    img = rng_tensor(61, (2, 3, 224, 224))
    for l, P in enumerate(ref_probs(sd, img)):
        dist = R.stats(P.numpy(), 14, 14)[..., 0].mean(axis=0)               # (H,) per-head distance, mean over the images
        spread = float((dist.max() - dist.min()) / dist.mean())
        print(f"block {l}: per-head distance {dist.min():.2f} .. {dist.max():.2f}, spread {spread:.3f} of the mean")
        assert spread >= 0.10
