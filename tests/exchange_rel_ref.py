"""float64 reference of the Fus_CrossViT exchange maps and the cross-stream relevance (include/mfvit.h: mfvit_fusion_ex_attention,
mfvit_fusion_ex_grad_attention, mfvit_bimodal_relevance).  Test infrastructure only; torch on the CPU.

  * fus_forward_probs: Fus_CrossViT.forward from features with oracle.ref_fusion.cross_attention restated so that every exchange layer's softmax
    probabilities are kept (retain_grad) - direction "cxr" is the CXR cls query (block [0], keys: its own cls token, then the ENH patches).
  * abar_of: the gradient-weighted map from autograd, mean over heads of max(0, a o d y / d a).
  * explicit_cross_relevance: the definition with R_s and Rbar_s as full T x T matrices.
  * chain_cross_relevance: the same quantities as vector chains (cls row, row sums, seeded row) - the form the GPU kernel runs - with switches
    that break it on purpose for the mutation checks.
"""
import torch

from oracle import ref_vit


def rel_err(got, ref):
    ref, got = ref.detach().double().cpu(), got.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def ref_features(p, img, heads):
    """float64 features3D with every block's probabilities (B, H, T, T) kept for their gradient (oracle.ref_vit's block restated)."""
    x = ref_vit.patch_embed(p, img)
    x = torch.cat([p["cls_token"].expand(x.shape[0], -1, -1), x], dim=1) + p["pos_embed"]
    probs = []
    for i in range(ref_vit.depth_of(p)):
        pre = f"blocks.{i}."
        y = ref_vit.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], ref_vit.LN_EPS)
        B, T, D = y.shape
        d = D // heads
        qkv = (y @ p[pre + "attn.qkv.weight"].t() + p[pre + "attn.qkv.bias"]).reshape(B, T, 3, heads, d).permute(2, 0, 3, 1, 4)
        P = (qkv[0] @ qkv[1].transpose(-2, -1) * d ** -0.5).softmax(dim=-1)
        P.retain_grad()
        probs.append(P)
        o = (P @ qkv[2]).transpose(1, 2).reshape(B, T, D)
        x = x + o @ p[pre + "attn.proj.weight"].t() + p[pre + "attn.proj.bias"]
        y = ref_vit.layer_norm(x, p[pre + "norm2.weight"], p[pre + "norm2.bias"], ref_vit.LN_EPS)
        h = ref_vit.gelu_erf(y @ p[pre + "mlp.fc1.weight"].t() + p[pre + "mlp.fc1.bias"])
        x = x + h @ p[pre + "mlp.fc2.weight"].t() + p[pre + "mlp.fc2.bias"]
    return ref_vit.layer_norm(x, p["norm.weight"], p["norm.bias"], ref_vit.LN_EPS), probs


def encoder_maps(probs):
    """A_l = mean over heads of max(0, P o d y / d P) of every block, after the score's backward."""
    return [(P * P.grad).clamp(min=0).mean(dim=1).detach() for P in probs]


def fus_forward_probs(p, fc, fe, heads=3, L=1, pool="cls", M=1):
    """Fus_CrossViT.forward (FUS:126-157) from features: (fused (B, C), [(a_cxr, a_enh) of every exchange layer], the retained
    (B, heads, 1, T) probability tensors)."""
    ln = ref_vit.layer_norm
    xs, xl = fc, fe
    kept = []
    for l in range(L):
        P = f"multi_scale_transformers.{M - 1}.cross_attn_layers.{l}."
        sc, x_small, lc, x_large = xs[:, :1], xs[:, 1:], xl[:, :1], xl[:, 1:]
        y = ln(torch.cat((lc, x_small), 1), p[P + "2.norm.weight"], p[P + "2.norm.bias"], 1e-5)
        o_l, a_enh = cross_attention_probs(p, P + "2.fn.", y, heads)
        xl_n = ln(torch.cat((lc + o_l, x_large), 1), p[P + "1.weight"], p[P + "1.bias"], 1e-6)
        y = ln(torch.cat((sc, x_large), 1), p[P + "0.norm.weight"], p[P + "0.norm.bias"], 1e-5)
        o_s, a_cxr = cross_attention_probs(p, P + "0.fn.", y, heads)
        xs_n = ln(torch.cat((sc + o_s, x_small), 1), p[P + "3.weight"], p[P + "3.bias"], 1e-6)
        kept.append((a_cxr, a_enh))
        xs, xl = xs_n, xl_n
    cf, ef = fc + xs, fe + xl
    cc, ec = (cf.mean(1), ef.mean(1)) if pool == "mean" else (cf[:, 0], ef[:, 0])
    fused = (cc @ p["mlp_head_cxr.0.weight"].t() + p["mlp_head_cxr.0.bias"]) + (ec @ p["mlp_head_enh.0.weight"].t() + p["mlp_head_enh.0.bias"])
    return fused, kept


def cross_attention_probs(p, pre, x, heads):
    """oracle.ref_fusion.cross_attention (module.py:123-137) with the probabilities kept: ((B, 1, C) output, the retained (B, heads, 1, N)
    probability tensor, whose .grad the score's backward fills)."""
    B, N, C = x.shape
    d = C // heads
    q = (x[:, 0:1] @ p[pre + "wq.weight"].t()).reshape(B, 1, heads, d).permute(0, 2, 1, 3)
    k = (x @ p[pre + "wk.weight"].t()).reshape(B, N, heads, d).permute(0, 2, 1, 3)
    v = (x @ p[pre + "wv.weight"].t()).reshape(B, N, heads, d).permute(0, 2, 1, 3)
    a = ((q @ k.transpose(-2, -1)) * (d ** -0.5)).softmax(dim=-1)
    if a.requires_grad:
        a.retain_grad()
    o = (a @ v).transpose(1, 2).reshape(B, 1, C)
    return o @ p[pre + "proj.weight"].t() + p[pre + "proj.bias"], a


def abar_of(a, drop_last_head=False):
    """(B, T) = (1 / H) sum_h max(0, a_h o d y / d a_h) of a retained (B, H, 1, T) probability tensor after the score's backward.
    drop_last_head (mutation): the last head is left out of the sum."""
    t = (a * a.grad).clamp(min=0)[:, :, 0].detach()
    H = t.shape[1]
    return (t[:, :-1] if drop_last_head else t).sum(dim=1) / H


# ------------------------------------------------------------------------------------------------ part 3, explicit T x T form
def _R(A):
    """R = (I + A_{L-1}) ... (I + A_0) of one image: A a list of (T, T)."""
    T = A[0].shape[-1]
    R = torch.eye(T, dtype=A[0].dtype)
    for a in A:
        R = R + a @ R
    return R


def _Rbar(R):
    T = R.shape[0]
    I = torch.eye(T, dtype=R.dtype)
    n = (R - I).sum(dim=1)
    out = I.clone()
    for j in range(T):
        if n[j] > 0:
            out[j] = (R[j] - I[j]) / n[j] + I[j]
    return out, n


def explicit_cross_relevance(A_c, A_e, abar_c, abar_e):
    """A_s: list over blocks of (B, T, T); abar_s (B, T) (abar_c: the CXR cls query's map).  -> (rel_cc, rel_ce, rel_ec, rel_ee), (B, T-1) each."""
    B = abar_c.shape[0]
    outs = [[], [], [], []]
    for b in range(B):
        R_c, R_e = _R([a[b] for a in A_c]), _R([a[b] for a in A_e])
        Rb_c, _ = _Rbar(R_c)
        Rb_e, _ = _Rbar(R_e)
        w0, w1 = abar_c[b].clone(), abar_e[b].clone()
        w0[0] = 0
        w1[0] = 0
        outs[0].append((1 + abar_c[b, 0]) * R_c[0, 1:])
        outs[1].append(Rb_c[0, 0] * (w0 @ Rb_e)[1:])
        outs[2].append(Rb_e[0, 0] * (w1 @ Rb_c)[1:])
        outs[3].append((1 + abar_e[b, 0]) * R_e[0, 1:])
    return tuple(torch.stack(o) for o in outs)


# ------------------------------------------------------------------------------------------------ part 3, chain form
def _chains(A, w, normalise=True):
    """One image, one stream: (r, n, what R - what + w) from three vector chains over A (list of (T, T)); w (T,) with w[0] = 0.
    normalise=False (mutation): what = w and the seeded row is w R."""
    T = A[0].shape[-1]
    r = torch.zeros(T, dtype=A[0].dtype)
    r[0] = 1
    for a in reversed(A):
        r = r + r @ a
    c = torch.ones(T, dtype=A[0].dtype)
    for a in A:
        c = c + a @ c
    n = c - 1
    if normalise:
        what = torch.where(n > 0, w / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(w))
    else:
        what = w.clone()
    x = what.clone()
    for a in reversed(A):
        x = x + x @ a
    return r, n, (x - what + w if normalise else x)


def chain_cross_relevance(A_c, A_e, abar_c, abar_e, normalise=True, own_cls_term=True, swap=False):
    """explicit_cross_relevance computed with the vector chains.  Mutations: normalise=False drops every division by n (what = w, Rbar[0,0] = r[0]),
    own_cls_term=False drops the (1 + Abar[0]) factor, swap exchanges the two directions' maps."""
    if swap:
        abar_c, abar_e = abar_e, abar_c
    B = abar_c.shape[0]
    outs = [[], [], [], []]
    for b in range(B):
        w0, w1 = abar_c[b].clone(), abar_e[b].clone()
        w0[0] = 0
        w1[0] = 0
        r_c, n_c, x_c = _chains([a[b] for a in A_c], w1, normalise)      # ENH cls -> CXR patches runs through R_c
        r_e, n_e, x_e = _chains([a[b] for a in A_e], w0, normalise)

        def rb00(r, n):
            if not normalise:
                return r[0]
            return (r[0] - 1) / n[0] + 1 if n[0] > 0 else torch.ones((), dtype=r.dtype)
        outs[0].append((1 + abar_c[b, 0] if own_cls_term else 1) * r_c[1:])
        outs[1].append(rb00(r_c, n_c) * x_e[1:])
        outs[2].append(rb00(r_e, n_e) * x_c[1:])
        outs[3].append((1 + abar_e[b, 0] if own_cls_term else 1) * r_e[1:])
    return tuple(torch.stack(o) for o in outs)


def synthetic_maps(seed, L, B, T, scale=0.02, zero_token=None):
    """L non-negative (B, T, T) float64 maps, uniform in [0, scale); zero_token: a token whose rows are zero in every map (n = 0 there)."""
    g = torch.Generator().manual_seed(seed)
    A = [torch.rand(B, T, T, generator=g, dtype=torch.float64) * scale for _ in range(L)]
    if zero_token is not None:
        for a in A:
            a[:, zero_token, :] = 0
    return A
