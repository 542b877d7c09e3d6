"""float64 restatement of the image encoder under patch dropout (timm >= 0.9 ``PatchDropout(prob, num_prefix_tokens=1)``; Liu et al. 2022):

    x = cat(cls, patch_embed(img)) + pos_embed  ->  keep cls and the patch rows idx[b, :]  ->  blocks  ->  final LayerNorm

composed from the pieces of the unchanged oracle (oracle/ref_vit.py: patch_embed, block / mhsa, layer_norm), gradients by autograd.  Also here:
the inputs the GPU tests run on (CASES, shared with the CPU test that bounds the restatement's own float32 error on them), timm's draw, and
deliberately wrong variants of the restatement (MUTATIONS) that the gates must tell from the right one."""
import functools

import numpy as np
import torch

from oracle import ref_vit

HEADS = ref_vit.HEADS
# the gates the project already applies to the undropped encoder (tests/test_encoder_gpu.py:42,61; tests/test_precision_gpu.py:388-452), as
# (features / logits, gradients) on the scale_err measure of tests/test_encoder_gpu.py
CAPS = {"fp32": (1e-3, 2e-3), "bf16": (4e-2, 6e-2), "bf16x3": (1e-3, 1e-3), "fp16": (6e-3, 2e-2)}


def scale_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def num_keep(L, prob):
    return max(1, int(L * (1.0 - prob)))


def draw_indices(B, L, prob, ordered=False, device="cpu"):
    """timm's PatchDropout draw."""
    idx = torch.argsort(torch.randn(B, L, device=device), dim=-1)[:, :num_keep(L, prob)]
    return idx.sort(dim=-1)[0] if ordered else idx


def rng(seed, shape):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).float()


def rng_indices(seed, B, L, K, ordered=False):
    """(B, K) distinct patch indices per image, a different unordered set for every sample (numpy PCG64: platform-independent)."""
    g = np.random.Generator(np.random.PCG64(seed))
    idx = torch.from_numpy(np.stack([g.permutation(L)[:K] for _ in range(B)])).long()
    return idx.sort(dim=-1)[0] if ordered else idx


def params_for(seed, hw, depth, num_classes=3):
    """Seeded weights of a vit_small of `depth` blocks for an (H, W) input: the oracle's recipe, pos_embed the sin-cos table of the grid."""
    h, w = hw
    p = ref_vit.seeded_params(seed, num_classes=num_classes, depth=depth, img_size=h)
    if h != w:
        p["pos_embed"] = ref_vit.sincos_pos_embed(h // 16, w // 16, p["cls_token"].shape[-1])
    return p


# --------------------------------------------------------------------------------------------------- the restatement
def embed(p, img):
    B = img.shape[0]
    return torch.cat([p["cls_token"].expand(B, -1, -1), ref_vit.patch_embed(p, img)], dim=1) + p["pos_embed"]


def keep_rows(x, idx):
    """cls and the patch rows idx (B, K) of x (B, 1 + L, D)."""
    B, _, D = x.shape
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + idx], dim=1)
    return torch.gather(x, 1, rows[:, :, None].expand(-1, -1, D))


def block_scaled(p, i, x, heads, s_attn, s_mlp):
    """ref_vit.block with per-sample factors (B,) on the two residual branches (timm drop_path: 0 or 1 / (1 - rate))."""
    pre = f"blocks.{i}."
    x = x + s_attn[:, None, None] * ref_vit.mhsa(p, pre, ref_vit.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], ref_vit.LN_EPS), heads)
    y = ref_vit.layer_norm(x, p[pre + "norm2.weight"], p[pre + "norm2.bias"], ref_vit.LN_EPS)
    h = ref_vit.gelu_erf(ref_vit.mm(y, p[pre + "mlp.fc1.weight"].t()) + p[pre + "mlp.fc1.bias"])
    return x + s_mlp[:, None, None] * (ref_vit.mm(h, p[pre + "mlp.fc2.weight"].t()) + p[pre + "mlp.fc2.bias"])


def features3d_keep(p, img, idx, heads=HEADS, path_factors=None):
    """(B, 1 + K, D) features under patch dropout.  path_factors: None, or (depth, 2, B) per-sample factors of the attention / MLP branch."""
    x = keep_rows(embed(p, img), idx)
    for i in range(ref_vit.depth_of(p)):
        x = ref_vit.block(p, i, x, heads) if path_factors is None else block_scaled(p, i, x, heads, path_factors[i, 0], path_factors[i, 1])
    return ref_vit.layer_norm(x, p["norm.weight"], p["norm.bias"], ref_vit.LN_EPS)


# --------------------------------------------------------------------------------------------------- wrong variants (tests only)
def _mut_pos(p, img, idx, heads=HEADS):
    """pos_embed[1 + k] instead of pos_embed[1 + idx[b, k]]: the position table added AFTER the gather."""
    B, K = idx.shape
    x = torch.cat([p["cls_token"].expand(B, -1, -1), ref_vit.patch_embed(p, img)], dim=1)
    x = keep_rows(x, idx) + p["pos_embed"][:, :1 + K]
    for i in range(ref_vit.depth_of(p)):
        x = ref_vit.block(p, i, x, heads)
    return ref_vit.layer_norm(x, p["norm.weight"], p["norm.bias"], ref_vit.LN_EPS)


def _mut_sample0(p, img, idx, heads=HEADS):
    """sample 0's indices used for every sample."""
    return features3d_keep(p, img, idx[:1].expand_as(idx), heads)


def _mut_swap(p, img, idx, heads=HEADS):
    """row and column swapped in the patch index: idx read column-major over the (gh, gw) grid."""
    gh, gw = img.shape[2] // 16, img.shape[3] // 16
    return features3d_keep(p, img, (idx % gh) * gw + idx // gh, heads)


MUTATIONS = {"pos_after_gather": _mut_pos, "sample0_indices": _mut_sample0, "row_col_swapped": _mut_swap}


def dimg_not_zeroed(dimg, idx):
    """A d img whose dropped patches were not zeroed: they hold the first kept patch's gradient of their image."""
    B, C, H, W = dimg.shape
    gh, gw = H // 16, W // 16
    pt = dimg.reshape(B, C, gh, 16, gw, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, -1).clone()
    for b in range(B):
        kept = torch.zeros(gh * gw, dtype=torch.bool)
        kept[idx[b]] = True
        pt[b, ~kept] = pt[b, idx[b, 0]].clone()
    return pt.reshape(B, gh, gw, C, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def dropped_mask(idx, hw):
    """(B, 1, H, W) bool: True on the pixels of the dropped patches."""
    gh, gw = hw[0] // 16, hw[1] // 16
    B = idx.shape[0]
    kept = torch.zeros(B, gh * gw, dtype=torch.bool)
    kept.scatter_(1, idx, True)
    return (~kept).reshape(B, 1, gh, 1, gw, 1).expand(B, 1, gh, 16, gw, 16).reshape(B, 1, hw[0], hw[1])


# --------------------------------------------------------------------------------------------------- the inputs of the GPU tests
# name -> (H, W), depth, B, K, ordered, with gradients.  The smallest shapes at which the index math and the kernel families can go wrong:
# L = 16; a non-square grid; 224^2 at T = 2, K = L - 1, K = L, one past a 64-row chunk and a 128-row block; B = 43 at depth 1 (516 (image, head)
# pairs: at 5 - 7 row tiles the persistent attention forward, at 7 the single-pass backward of the split / 16-bit types - the only family
# switches mfvit_attention_plan reports between T = 2 and 197, tests/test_patch_drop_cpu.py asserts it).
CASES = {
    "sq64": ((64, 64), 2, 2, 8, False, True),
    "sq64_ordered": ((64, 64), 2, 3, 5, True, True),
    "rect96x64": ((96, 64), 2, 3, 11, False, True),
    "t2": ((224, 224), 1, 2, 1, False, True),
    "k64": ((224, 224), 1, 2, 64, False, True),
    "k128": ((224, 224), 1, 2, 128, False, True),
    "k195": ((224, 224), 1, 2, 195, False, True),
    "k196": ((224, 224), 1, 2, 196, False, True),
    "b43_t128": ((224, 224), 1, 43, 127, False, False),
    "b43_t129": ((224, 224), 1, 43, 128, False, False),
    "b43_t192": ((224, 224), 1, 43, 191, False, True),
    "b43_t193": ((224, 224), 1, 43, 192, False, True),
}
_SEED = {name: 9100 + 10 * i for i, name in enumerate(CASES)}


def case_inputs(name, num_classes=3):
    """(params, img, idx, feature weights, logit weights) of a case, float32 on the CPU."""
    hw, depth, B, K, ordered, _ = CASES[name]
    s = _SEED[name]
    L = (hw[0] // 16) * (hw[1] // 16)
    return (params_for(s, hw, depth, num_classes), rng(s + 1, (B, 3) + hw), rng_indices(s + 2, B, L, K, ordered),
            rng(s + 3, (B, 1 + K, 384)), rng(s + 4, (B, num_classes)))


def run(p, img, idx, r, rl, dtype, fn=features3d_keep, grads=True, stop_grad_conv1=False, img_grad=True, **kw):
    """Features, logits and (grads) the gradients of loss = sum(features * r) + sum(logits * rl) in `dtype`."""
    pd = {k: v.to(dtype).requires_grad_(grads and k != "pos_embed" and not (stop_grad_conv1 and k.startswith("patch_embed"))) for k, v in p.items()}
    x = img.to(dtype).requires_grad_(grads and img_grad)
    with torch.set_grad_enabled(grads):
        f = fn(pd, x, idx, **kw)
        logits = ref_vit.head_linear(pd, f[:, 0])
        if grads:
            ((f * r.to(dtype)).sum() + (logits * rl.to(dtype)).sum()).backward()
    out = {"features": f.detach(), "logits": logits.detach()}
    if grads:
        out["grads"] = {k: v.grad for k, v in pd.items() if v.grad is not None}
        out["dimg"] = x.grad
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a case: computed once, shared by every test that needs it.  Treat as read-only."""
    p, img, idx, r, rl = case_inputs(name)
    return run(p, img, idx, r, rl, torch.float64, grads=CASES[name][5])
