"""float64 restatement of attention-guided token pruning between the blocks of the image encoder (include/mfvit.h, mfvit_token_*; Liang et al.
2022, "Not All Patches Are What You Need": EViT's token reorganisation - here at a block boundary, with normalised weights that are constants
of the backward).  Behind block l of `prune_blocks`, on x_{l+1} (B, T, D), row 0 = cls:

    s[b, j]  = mean over heads of softmax(q k^T / sqrt(d))[b, h, 0, 1 + j]        block l's own attention, j in [0, T - 1)
    K        = ceil(keep_rate (T - 1));  K == T - 1: the stage is skipped
    keep     = {j : rank[j] < K}, ascending; rank = position by (value descending, index ascending, NaN last)
    x'       = cat(cls row, kept rows, [sum over the dropped j of w_j x_{l+1}[1 + j]]),   w_j = s_j / sum_dropped s  (1 / n_dropped when that sum
               is zero or not finite); w and the selection carry no gradient

composed from the unchanged oracle (oracle/ref_vit.py: block, layer_norm, mm) and tests/patch_drop_ref.py (embed, keep_rows, seeded inputs, CAPS,
scale_err), gradients by autograd.  Also here: numpy references of the four kernels, the inputs of the GPU tests (CASES; the seeds are chosen so
that the K-th and (K+1)-th score of every image and stage lie at least 1e-3 apart, relatively: tests/test_token_prune_cpu.py lists the gaps), and
deliberately wrong variants (MUTATIONS) the gates must tell from the right one."""
import functools
import math

import numpy as np
import torch

import patch_drop_ref as P
from oracle import ref_vit

HEADS = ref_vit.HEADS
CAPS = P.CAPS
scale_err = P.scale_err
rng = P.rng


# --------------------------------------------------------------------------------------------------- host logic
def num_keep(T, rate):
    """K of a stage on T rows (cls included)."""
    return max(1, min(T - 1, int(math.ceil(rate * (T - 1)))))


def token_schedule(T, depth, blocks, rate, fuse):
    """Tokens per segment: [T_0, T_1, ..] with a new entry behind every block of `blocks` whose stage is not skipped."""
    out = [T]
    if rate >= 1.0:
        return out
    for l in blocks:
        K = num_keep(out[-1], rate)
        if K < out[-1] - 1:
            out.append(1 + K + int(bool(fuse)))
    return out


# --------------------------------------------------------------------------------------------------- kernel-level references (numpy)
def rank_ref(score):
    """(B, P) -> int rank, the order of mfvit_patch_rank: value descending, ties to the lower index, NaN last, -0.0 == +0.0."""
    s = np.asarray(score, dtype=np.float64) + 0.0
    order = np.argsort(-s, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(s.shape[1]), s.shape), axis=1)
    return rank


def select_ref(score, K, dtype=np.float32):
    """score (B, P) -> idx_keep (B, K), idx_drop (B, P - K), both ascending, w (B, P - K): the dropped scores over their sum, added in ascending
    order in `dtype` (float32: the kernel's own arithmetic, to the bit)."""
    s = np.asarray(score, dtype=dtype)
    B, Pn = s.shape
    kept = rank_ref(s) < K
    keep = np.stack([np.nonzero(kept[b])[0] for b in range(B)]).astype(np.int64).reshape(B, K)
    drop = np.stack([np.nonzero(~kept[b])[0] for b in range(B)]).astype(np.int64).reshape(B, Pn - K)
    w = np.zeros((B, Pn - K), dtype=dtype)
    for b in range(B):
        if Pn == K:
            break
        d = s[b, drop[b]]
        tot = d[0]
        for v in d[1:]:
            tot = dtype(tot + v)
        with np.errstate(all="ignore"):
            w[b] = dtype(1.0) / dtype(Pn - K) if (tot == 0 or not np.isfinite(tot)) else d / tot
    return keep, drop, w


def reorg_fwd_ref(x, keep, drop, w, fuse):
    """float64 value of the forward on f32 inputs: (B, T, D) -> (B, 1 + K + fuse, D)."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    rows = [x[:, :1], np.stack([x[b, 1 + keep[b]] for b in range(B)])]
    if fuse:
        rows.append(np.stack([(np.asarray(w[b], dtype=np.float64)[:, None] * x[b, 1 + drop[b]]).sum(0) for b in range(B)])[:, None])
    return np.concatenate(rows, axis=1)


def reorg_fwd_abs(x, drop, w):
    """(B, D): sum over the dropped rows of |w_j x_j| - the scale of the fused row's rounding error."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.stack([(np.abs(np.asarray(w[b], dtype=np.float64))[:, None] * x[b, 1 + drop[b]]).sum(0) for b in range(x.shape[0])])


def reorg_bwd_ref(dout, keep, drop, w, T, fuse):
    """f32, to the bit: cls and kept rows moved back, a dropped row = w_j * dout[fused] (one f32 product), zeros otherwise."""
    dout = np.asarray(dout, dtype=np.float32)
    B, _, D = dout.shape
    K = keep.shape[1]
    dx = np.zeros((B, T, D), dtype=np.float32)
    dx[:, 0] = dout[:, 0]
    for b in range(B):
        dx[b, 1 + keep[b]] = dout[b, 1:1 + K]
        if fuse:
            dx[b, 1 + drop[b]] = np.asarray(w[b], dtype=np.float32)[:, None] * dout[b, 1 + K][None]
    return dx


# --------------------------------------------------------------------------------------------------- the restatement (torch, any dtype)
def cls_score(p, l, x, heads=HEADS):
    """(B, T - 1): the cls row of block l's attention on its input x = x_l, mean over the heads, cls column dropped.  No gradient."""
    with torch.no_grad():
        pre = f"blocks.{l}."
        y = ref_vit.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], ref_vit.LN_EPS)
        B, T, D = y.shape
        d = D // heads
        qkv = (ref_vit.mm(y, p[pre + "attn.qkv.weight"].t()) + p[pre + "attn.qkv.bias"]).reshape(B, T, 3, heads, d).permute(2, 0, 3, 1, 4)
        a = (ref_vit.mm(qkv[0][:, :, :1], qkv[1].transpose(-2, -1)) * d ** -0.5).softmax(dim=-1)       # (B, h, 1, T)
        return a[:, :, 0, 1:].mean(dim=1)


def select(s, K):
    """s (B, P) torch -> (idx_keep, idx_drop) int64, ascending: the K best by (value descending, index ascending)."""
    keep, drop, _ = select_ref(s.detach().double().numpy(), K, dtype=np.float64)
    return torch.from_numpy(keep), torch.from_numpy(drop)


def drop_of(keep, Pn):
    """The ascending complement of keep (B, K) in [0, Pn)."""
    m = torch.ones(keep.shape[0], Pn, dtype=torch.bool)
    m.scatter_(1, keep, False)
    return torch.stack([torch.nonzero(m[b])[:, 0] for b in range(keep.shape[0])]).reshape(keep.shape[0], Pn - keep.shape[1])


def weights(s, drop):
    sd = torch.gather(s, 1, drop)
    tot = sd.sum(dim=1, keepdim=True)
    bad = (tot == 0) | ~torch.isfinite(tot)
    return torch.where(bad, torch.full_like(sd, 1.0 / drop.shape[1]), sd / torch.where(bad, torch.ones_like(tot), tot)).detach()


def rows_of(x, idx):
    return torch.gather(x, 1, (1 + idx)[:, :, None].expand(-1, -1, x.shape[2]))


def reorg(x, s, keep, fuse, normalise=True, sort_keep=True, with_fused=True):
    """x (B, T, D), s (B, T - 1), keep (B, K) -> (B, 1 + K + fuse, D).  The three switches are the mutations' (all True: the definition)."""
    drop = drop_of(keep, x.shape[1] - 1)
    if sort_keep:
        keep = keep.sort(dim=1)[0]
    parts = [x[:, :1], rows_of(x, keep)]
    if fuse:
        w = weights(s, drop) if normalise else torch.gather(s, 1, drop).detach()
        fused = (w[:, :, None] * rows_of(x, drop)).sum(dim=1, keepdim=True)
        parts.append(fused if with_fused else torch.zeros_like(fused))
    return torch.cat(parts, dim=1)


def block_masked(p, i, x, heads, mk, rates):
    """timm's training-mode block with the given keep masks (tests/test_vit_dropout_gpu.py: ref_logits) - mk: {(site name, block): mask}."""
    drop, attn, dpr = rates

    def dr(t, key, rate):
        return t * mk[key] / (1.0 - rate) if key in mk else t
    pre = f"blocks.{i}."
    y = ref_vit.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], ref_vit.LN_EPS)
    B, T, D = y.shape
    hd = D // heads
    qkv = (y @ p[pre + "attn.qkv.weight"].t() + p[pre + "attn.qkv.bias"]).reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = dr(((qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1), ("attn", i), attn)
    o = (a @ qkv[2]).transpose(1, 2).reshape(B, T, D) @ p[pre + "attn.proj.weight"].t() + p[pre + "attn.proj.bias"]
    x = x + dr(dr(o, ("proj", i), drop), ("dp_attn", i), dpr[i])
    y = ref_vit.layer_norm(x, p[pre + "norm2.weight"], p[pre + "norm2.bias"], ref_vit.LN_EPS)
    h = dr(ref_vit.gelu_erf(y @ p[pre + "mlp.fc1.weight"].t() + p[pre + "mlp.fc1.bias"]), ("gelu", i), drop)
    o = h @ p[pre + "mlp.fc2.weight"].t() + p[pre + "mlp.fc2.bias"]
    return x + dr(dr(o, ("fc2", i), drop), ("dp_mlp", i), dpr[i])


def features3d_pruned(p, img, blocks, rate, fuse=True, indices=None, patch_idx=None, heads=HEADS, masks=None, rates=None, num_keep_fn=num_keep,
                      reorg_fn=reorg):
    """(features (B, T_last, D), [idx_keep (B, K) of every executed stage, in that stage's own row numbering]).  indices: the selections to use
    (same structure) instead of the restatement's own; patch_idx: patch dropout in front (tests/patch_drop_ref.py); masks / rates: the keep masks
    of a training-mode forward with dropout, as block_masked takes them (masks["pos"]: pos_drop)."""
    x = P.embed(p, img)
    if patch_idx is not None:
        x = P.keep_rows(x, patch_idx)
    if masks is not None and "pos" in masks:
        x = x * masks["pos"] / (1.0 - rates[0])
    sel = []
    for i in range(ref_vit.depth_of(p)):
        x_in = x
        x = ref_vit.block(p, i, x, heads) if masks is None else block_masked(p, i, x, heads, masks, rates)
        if rate < 1.0 and i in blocks:
            T = x.shape[1]
            K = num_keep_fn(T, rate)
            if K >= T - 1:
                continue
            s = cls_score(p, i, x_in.detach(), heads)
            keep = indices[len(sel)] if indices is not None else select(s, K)[0]
            x = reorg_fn(x, s, keep, fuse)
            sel.append(keep)
    return ref_vit.layer_norm(x, p["norm.weight"], p["norm.bias"], ref_vit.LN_EPS), sel


def token_origin(sel, T0, fuse):
    """(B, T_last - 1) original row indices (0-based, cls not counted) of the rows behind the stages `sel`; -1: a fused row."""
    B = sel[0].shape[0] if sel else 1
    org = torch.arange(T0 - 1).expand(B, -1)
    for keep in sel:
        org = torch.gather(org, 1, keep.sort(dim=1)[0])
        if fuse:
            org = torch.cat([org, torch.full((B, 1), -1, dtype=org.dtype)], dim=1)
    return org


# --------------------------------------------------------------------------------------------------- wrong variants (tests only)
MUTATIONS = {
    "unnormalised_weights": dict(reorg_fn=lambda x, s, keep, fuse: reorg(x, s, keep, fuse, normalise=False)),
    "no_fused_row": dict(reorg_fn=lambda x, s, keep, fuse: reorg(x, s, keep, fuse, with_fused=False)),
    "rank_order": dict(reorg_fn=lambda x, s, keep, fuse: reorg(
        x, s, torch.gather(keep, 1, torch.argsort(-torch.gather(s, 1, keep), dim=1, stable=True)), fuse, sort_keep=False)),
    "sample0_indices": dict(reorg_fn=lambda x, s, keep, fuse: reorg(x, s, keep[:1].expand_as(keep), fuse)),
    "floor_K": dict(num_keep_fn=lambda T, rate: max(1, int(math.floor(rate * (T - 1))))),
}


class _NoFusedGrad(torch.autograd.Function):
    """identity whose backward drops the gradient: the fused row's gradient not distributed"""
    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


def _reorg_fused_grad_lost(x, s, keep, fuse):
    out = reorg(x, s, keep, fuse)
    return torch.cat([out[:, :-1], _NoFusedGrad.apply(out[:, -1:])], dim=1) if fuse else out


MUTATIONS["fused_grad_not_distributed"] = dict(reorg_fn=_reorg_fused_grad_lost)


# --------------------------------------------------------------------------------------------------- the inputs of the GPU tests
# name -> dict(hw, depth, B, heads, dim, blocks, rate, fuse, patch_keep (K of a patch dropout in front, or None), seed).  The smallest shapes at
# which each piece can go wrong: two stages with a fused row among the candidates of the second (37 -> 20 -> 12), 6 heads of 64 at rate 0.7, a
# sequence that crosses the 128-row tile (197 -> 140), dim 768, no fused row, patch dropout in front.  The seeds: see the module docstring.
CASES = {
    "two_stage96": dict(hw=(96, 96), depth=4, B=3, heads=12, dim=384, blocks=(0, 2), rate=0.5, fuse=True, patch_keep=None, seed=9900),
    "heads6_64": dict(hw=(64, 64), depth=3, B=2, heads=6, dim=384, blocks=(0, 1), rate=0.7, fuse=True, patch_keep=None, seed=9910),
    "tile224": dict(hw=(224, 224), depth=2, B=2, heads=12, dim=384, blocks=(0,), rate=0.7, fuse=True, patch_keep=None, seed=9920),
    "base768": dict(hw=(64, 64), depth=2, B=2, heads=12, dim=768, blocks=(0,), rate=0.5, fuse=True, patch_keep=None, seed=9930),
    "nofuse96": dict(hw=(96, 96), depth=3, B=2, heads=12, dim=384, blocks=(0, 1), rate=0.5, fuse=False, patch_keep=None, seed=9941),
    "patchdrop96": dict(hw=(96, 96), depth=3, B=2, heads=12, dim=384, blocks=(1,), rate=0.5, fuse=True, patch_keep=20, seed=9950),
}


def arch_of(c):
    return "vit_small" if c["dim"] == 384 else "vit_base"


def case_params(c, num_classes=3):
    h, w = c["hw"]
    p = ref_vit.seeded_params(c["seed"], arch=arch_of(c), num_classes=num_classes, depth=c["depth"], img_size=h)
    if h != w:
        p["pos_embed"] = ref_vit.sincos_pos_embed(h // 16, w // 16, c["dim"])
    return p


def case_inputs(name, patch=True, num_classes=3):
    """(params, img, patch_idx or None, feature weights, logit weights) of a case, float32 on the CPU.  patch=False: the case without its patch
    dropout (the model in eval())."""
    c = CASES[name]
    s, hw, B = c["seed"], c["hw"], c["B"]
    L = (hw[0] // 16) * (hw[1] // 16)
    pidx = P.rng_indices(s + 2, B, L, c["patch_keep"]) if (c["patch_keep"] and patch) else None
    T0 = 1 + (pidx.shape[1] if pidx is not None else L)
    T_last = token_schedule(T0, c["depth"], c["blocks"], c["rate"], c["fuse"])[-1]
    return case_params(c, num_classes), rng(s + 1, (B, 3) + hw), pidx, rng(s + 3, (B, T_last, c["dim"])), rng(s + 4, (B, num_classes))


def run(name, dtype, indices=None, grads=True, patch=True, **kw):
    """Features, logits, the selections and (grads) the gradients of loss = sum(features * r) + sum(logits * rl) of a case in `dtype`."""
    c = CASES[name]
    p, img, pidx, r, rl = case_inputs(name, patch)
    pd = {k: v.to(dtype).requires_grad_(grads and k != "pos_embed") for k, v in p.items()}
    x = img.to(dtype).requires_grad_(grads)
    with torch.set_grad_enabled(grads):
        f, sel = features3d_pruned(pd, x, c["blocks"], c["rate"], c["fuse"], indices=indices, patch_idx=pidx, heads=c["heads"], **kw)
        logits = ref_vit.head_linear(pd, f[:, 0])
        if grads:
            ((f * r.to(dtype)).sum() + (logits * rl.to(dtype)).sum()).backward()
    out = {"features": f.detach(), "logits": logits.detach(), "indices": sel}
    if grads:
        out["grads"] = {k: v.grad for k, v in pd.items() if v.grad is not None}
        out["dimg"] = x.grad
    return out


@functools.lru_cache(maxsize=None)
def reference(name, patch=True):
    """The float64 reference of a case with its own selection: computed once, shared by every test that needs it.  Treat as read-only."""
    return run(name, torch.float64, patch=patch)


def score_gaps(name, patch=True):
    """[(stage, image, relative gap between the K-th and (K+1)-th float64 score)] of a case."""
    c = CASES[name]
    p, img, pidx, _, _ = case_inputs(name, patch)
    pd = {k: v.double() for k, v in p.items()}
    gaps, stage = [], [0]

    def spy(x, s, keep, fuse):
        K = keep.shape[1]
        srt = s.sort(dim=1, descending=True)[0]
        gaps.extend((stage[0], b, float((srt[b, K - 1] - srt[b, K]) / srt[b, K - 1])) for b in range(s.shape[0]))
        stage[0] += 1
        return reorg(x, s, keep, fuse)
    with torch.no_grad():
        features3d_pruned(pd, img.double(), c["blocks"], c["rate"], c["fuse"], patch_idx=pidx, heads=c["heads"], reorg_fn=spy)
    return gaps
