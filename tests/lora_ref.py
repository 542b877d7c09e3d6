"""float64 references of the LoRA adapters (mfvit.lora, csrc/lora.hip), built on oracle.ref_vit / oracle.ref_fusion (imported, not changed).

An adapted Linear runs on W_eff = W + s B A; `merged` builds the oracle's parameter dict with exactly that (differentiable: torch autograd
through ref_vit.forward on the merged dict gives the adapters' gradients), q / k / v on their own row block of the fused attn.qkv.weight.
The elementwise gates of the two kernels are forward-error bounds of the stated f32 evaluation orders - nothing in them is measured.

split_floor, for the 'small update resolved' test of tests/test_lora_gpu.py (adapters at max|s B A| = 2^-8 max|W|, depth 12, B = 3): the
float64 oracle run once with the merged weights W + s B A rounded to the split-bf16 grid (hi = bf16(x), lo = bf16(x - hi), csrc/common.cuh)
and once unrounded; the floor is the largest |difference of the two runs' logits| relative to the largest |logits_adapted - logits_base| of the
unrounded oracle.  Recorded (CPU, the test's inputs): floor 5.64e-4, max|logits_adapted - logits_base| 1.03e-2; the test recomputes it (two
seconds) and asserts 4 x.  (With the BASE run's weights rounded as well and the two rounded runs subtracted - what the GPU's own difference
does - the figure is 4.28e-4; the MI355X measures 1.73e-3 for the difference, which also carries the activations' split rounding.)"""
import math

import torch

from oracle import ref_vit

TARGETS = ("q", "k", "v", "proj", "fc1", "fc2")
U = 2.0 ** -24          # unit roundoff of f32


def site(i, target):
    """(oracle key of the adapted weight, index of the row block or None, adapter key prefix, parameter suffix)."""
    if target in ("q", "k", "v"):
        return f"blocks.{i}.attn.qkv.weight", "qkv".index(target), f"blocks.{i}.attn.qkv.", "_" + target
    if target == "proj":
        return f"blocks.{i}.attn.proj.weight", None, f"blocks.{i}.attn.proj.", ""
    return f"blocks.{i}.mlp.{target}.weight", None, f"blocks.{i}.mlp.{target}.", ""


def items(blocks, targets):
    return [(i, t) for i in blocks for t in TARGETS if t in targets]


def shape_of(sd, i, target):
    key, rb, _, _ = site(i, target)
    N, K = sd[key].shape
    return (N // 3 if rb is not None else N), K


def seeded_adapters(seed, sd, rank, blocks, targets, s, ratio=2.0 ** -6):
    """{adapter state-dict key: f32 tensor}: A ~ U(+-1/sqrt(K)), B Gaussian, each B scaled so that max|s B A| = ratio max|W| of its own weight
    (row block)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i, t in items(blocks, targets):
        key, rb, pre, suf = site(i, t)
        N, K = shape_of(sd, i, t)
        a = (torch.rand(rank, K, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(K)
        b = torch.randn(N, rank, generator=g, dtype=torch.float64)
        w = sd[key].double()
        w = w[rb * N:(rb + 1) * N] if rb is not None else w
        b = b * (ratio * float(w.abs().max()) / float((s * (b @ a)).abs().max()))
        out[pre + "lora_A" + suf] = a.float()
        out[pre + "lora_B" + suf] = b.float()
    return out


def rescale(ad, factor):
    """The same adapters with every B multiplied by `factor` (max|s B A| scales with it)."""
    return {k: (v * factor if "lora_B" in k else v.clone()) for k, v in ad.items()}


def merged(pd, ad, s, blocks, targets):
    """The oracle's parameter dict with p[W] + s B @ A on the right row block of every item; ad: adapter tensors (any dtype, may require
    grad: torch autograd through ref_vit.forward on the result gives the adapters' gradients)."""
    out = dict(pd)
    for i, t in items(blocks, targets):
        key, rb, pre, suf = site(i, t)
        a, b = ad[pre + "lora_A" + suf].to(pd[key].dtype), ad[pre + "lora_B" + suf].to(pd[key].dtype)
        N = b.shape[0]
        upd = s * (b @ a)
        if rb is not None:
            z = torch.zeros_like(out[key])
            upd = torch.cat([z[:rb * N], upd, z[(rb + 1) * N:]], dim=0)
        out[key] = out[key] + upd
    return out


# ------------------------------------------------------------------ elementwise gates of the two kernels (f32 forward-error bounds)
def merge_ref_and_gate(w, a, b, s):
    """float64 w + s b a of the f32 inputs, and |got - ref| <= (r + 2) u (|w| + |s| sum_j |b| |a|): r fused multiply-adds (j ascending), one
    multiply by s, one add to w."""
    w, a, b = w.double(), a.double(), b.double()
    r = a.shape[0]
    ref = w + s * (b @ a)
    gate = (r + 2) * U * (w.abs() + abs(s) * (b.abs() @ a.abs()))
    return ref, gate


def grad_ref_and_gate(dw, a, b, s):
    """float64 (da, db) = (s b^T dw, s dw a^T) and their gates (terms + 2) u |s| sum |products| (terms = N for da, K for db): valid for
    any summation tree over `terms` products plus the multiply by s."""
    dw, a, b = dw.double(), a.double(), b.double()
    N, K = dw.shape
    da = s * (b.t() @ dw)
    db = s * (dw @ a.t())
    ga = (N + 2) * U * abs(s) * (b.abs().t() @ dw.abs())
    gb = (K + 2) * U * abs(s) * (dw.abs() @ a.abs().t())
    return (da, ga), (db, gb)


def within(got, ref, gate):
    """Largest |got - ref| / gate (<= 1 passes); an all-zero gate element demands exact equality."""
    d = (got.double().cpu() - ref).abs()
    ok_zero = bool(((gate == 0) <= (d == 0)).all())
    q = float((d / gate.clamp_min(1e-300)).max())
    return q if ok_zero else float("inf")


# ------------------------------------------------------------------ split-bf16 grid (csrc/common.cuh: hi = bf16(x), lo = bf16(x - hi))
def round_split_bf16(x):
    x32 = x.float()
    hi = x32.bfloat16().float()
    lo = (x32 - hi).bfloat16().float()
    return hi.double() + lo.double()


def split_floor(sd, ad, s, blocks, targets, img, heads=12):
    """(floor, d_ref): d_ref = the oracle's logits_adapted - logits_base (float64, unrounded weights); floor = the largest change of
    logits_adapted when every merged weight W + s B A is rounded to the split-bf16 grid first, relative to max|d_ref| - what the default
    precision's weight shadow cannot do better than."""
    pd = {k: v.double() for k, v in sd.items()}
    x = img.double()
    with torch.no_grad():
        m = merged(pd, ad, s, blocks, targets)
        adapted = ref_vit.forward(m, x, heads)
        d_ref = adapted - ref_vit.forward(pd, x, heads)
        keys = {site(i, t)[0] for i, t in items(blocks, targets)}
        rounded = ref_vit.forward({k: (round_split_bf16(v) if k in keys else v) for k, v in m.items()}, x, heads)
    return float((rounded - adapted).abs().max() / d_ref.abs().max()), d_ref
