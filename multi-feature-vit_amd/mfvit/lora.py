"""Low-rank adapters (LoRA, Hu et al. 2021) on the ViT encoders, for fine-tuning on a small labelled set.

An adapted Linear with frozen weight W (N x K) and adapters A (r x K), B (N x r) runs on the merged weight

    W_eff = W + s B A,    s = alpha / r   (alpha / sqrt(r) with rslora=True)

formed in f32 by one batched HIP launch (csrc/lora.hip) whenever a parameter or adapter version changes; the weight shadows
are built from W_eff, so every forward kernel - and everything that goes through ``_ensure_shadow``: attention maps,
relevance, attribution, ``Fus_CrossViT`` - sees the adapted model.  The backward is the exact chain rule through W_eff:
dW_eff = dY^T X from the weight-gradient GEMM of the adapted Linears only, then dB = s dW_eff A^T, dA = s B^T dW_eff.

Built for precision 'bf16x3' (the default) and 'fp32': a plain 16-bit shadow would round a young s B A away.
Not built: lora_dropout (no merged form), a rank-r weight gradient that never forms dW, DoRA / AdaLoRA, adapters
on the patch embedding, the fusion module, the TransFuser GPT or the MoCo builders, RCCL sync of adapter gradients.
"""
import itertools
import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import MfvitError, check, lib, ptr, stream

TARGETS = ("q", "k", "v", "proj", "fc1", "fc2")      # == MFVIT_LORA_Q .. MFVIT_LORA_FC2 (include/mfvit.h)
MAX_RANK = 64
_serial = itertools.count(1)


def _site(block, target):
    """(holder module, dotted name below the block, parameter suffix) of a target."""
    if target in ("q", "k", "v"):
        return block.attn.qkv, "attn.qkv", "_" + target
    if target == "proj":
        return block.attn.proj, "attn.proj", ""
    return getattr(block.mlp, target), "mlp." + target, ""


class LoraState:
    """What an encoder keeps while adapters are attached (``model._lora``): the items in a fixed order, the effective f32 arena
    (``eff``) its kernels read as `params`, and the dW_eff scratch (``dw``) of the selective backward."""

    def __init__(self, rank, alpha, rslora):
        self.rank, self.alpha, self.rslora = rank, float(alpha), bool(rslora)
        self.scale = self.alpha / math.sqrt(rank) if rslora else self.alpha / rank
        self.serial = next(_serial)
        self.items = []          # (block index, target code, holder module, name of A, name of B, full key prefix)
        self.base_flags = None   # requires_grad of every model parameter before add_lora touched them
        self.eff = None
        self.dw = None

    def named(self):
        """[(state-dict key, Parameter)]: A then B of every item, blocks ascending, targets in TARGETS order."""
        out = []
        for _, _, mod, na, nb, prefix in self.items:
            out += [(prefix + na, mod._parameters[na]), (prefix + nb, mod._parameters[nb])]
        return out

    def params(self):
        out = []
        for _, _, mod, na, nb, _ in self.items:
            out += [mod._parameters[na], mod._parameters[nb]]
        return out

    def new_grads(self, device):
        """Fresh gradient tensors, one per entry of params(): views of one flat f32 allocation."""
        ps = self.params()
        flat = torch.empty(sum(p.numel() for p in ps), device=device, dtype=torch.float32)
        return list(torch._utils._unflatten_dense_tensors(flat, ps))

    def request(self, grads=None):
        """mfvit_lora_req over the adapters as they are now (grads: the tensors of new_grads, or None for the forward side)."""
        ps = self.params()
        arr = (_lib.LoraItem * len(self.items))()
        for i, (blk, code, _, _, _, _) in enumerate(self.items):
            a, b = ps[2 * i], ps[2 * i + 1]
            if a.dtype != torch.float32 or b.dtype != torch.float32 or not a.is_contiguous() or not b.is_contiguous():
                raise MfvitError("LoRA adapters must stay contiguous float32 tensors")
            _lib.require_cuda(a, b)
            arr[i] = _lib.LoraItem(blk, code, a.data_ptr(), b.data_ptr(),
                                   grads[2 * i].data_ptr() if grads is not None else None,
                                   grads[2 * i + 1].data_ptr() if grads is not None else None)
        req = _lib.LoraReq(self.rank, self.scale, len(self.items), arr)
        req._keep = (arr, ps, grads)
        return req


def _encoder(model):
    from .encoder import VisionTransformerMoCo
    if not isinstance(model, VisionTransformerMoCo):
        raise NotImplementedError(f"LoRA adapters are built for the vits / vits_returnftrs image encoders (vit_small, vit_base), not for "
                                  f"{type(model).__name__}: the token-input GPT, the conv-stem variants (vit_conv_*), the fusion module and "
                                  "the MoCo builders are out of scope")
    return model


def has_lora(model):
    return getattr(model, "_lora", None) is not None


def _state(model):
    lo = getattr(_encoder(model), "_lora", None)
    if lo is None:
        raise ValueError("no LoRA adapters attached to this model (add_lora first)")
    return lo


def add_lora(model, rank=8, alpha=16.0, targets=("q", "v"), blocks=None, rslora=False, freeze_base=True, generator=None):
    """Attach rank-`rank` adapters to the Linears `targets` ('q', 'k', 'v': the three row blocks of the fused attn.qkv.weight, each
    with its own pair; 'proj', 'fc1', 'fc2') of the blocks `blocks` (indices, negative ones from the end; None: all).  New f32 leaf
    parameters on the adapted holders: blocks.{i}.attn.qkv.lora_A_q / lora_B_q (and _k, _v), blocks.{i}.attn.proj.lora_A / lora_B,
    blocks.{i}.mlp.fc1 / fc2.lora_A / lora_B.  A ~ U(-1/sqrt(K), 1/sqrt(K)) (kaiming_uniform_(a=sqrt(5)), as loralib; drawn on the CPU
    from `generator`), B = 0: the model's outputs are unchanged, bit for bit, until B moves.  freeze_base: requires_grad = False on
    every arena parameter (the head stays trainable); with a trainable arena parameter left the backward is the full one plus the
    contraction of the adapted dW - correct and slower.  Returns the adapter parameters.

    ValueError: rank outside 1..64, an unknown or repeated target, a block index out of range, adapters already attached.
    MfvitError: precision 'bf16' / 'fp16' (a plain 16-bit weight shadow rounds W_eff to 8 / 11 mantissa bits - a young s B A is below
    that resolution and would be rounded away; use 'bf16x3' or 'fp32').  NotImplementedError: anything but an image encoder."""
    m = _encoder(model)
    if has_lora(m):
        raise ValueError("LoRA adapters are already attached to this model (merge_lora or remove_lora first)")
    if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
        raise ValueError(f"rank must be an integer in 1..{MAX_RANK}, got {rank!r}")
    if isinstance(targets, str):
        targets = (targets,)
    targets = tuple(targets)
    if not targets or any(t not in TARGETS for t in targets) or len(set(targets)) != len(targets):
        raise ValueError(f"targets must be distinct names out of {TARGETS}, got {targets!r}")
    if not (isinstance(alpha, (int, float)) and math.isfinite(alpha)):
        raise ValueError(f"alpha must be a finite number, got {alpha!r}")
    blks = m._attn_blocks(blocks)           # (ValueError for an index out of range or an empty selection)
    if _lib.dtype_code(m.precision) in (_lib.BF16, _lib.F16):
        raise MfvitError(f"LoRA needs precision 'bf16x3' or 'fp32', this model runs {m.precision!r}: a plain 16-bit weight shadow rounds the "
                         "merged weight W + s B A to 8 / 11 mantissa bits, and a young low-rank update is below that resolution")
    lo = LoraState(rank, alpha, rslora)
    lo.base_flags = [(p, p.requires_grad) for p in m.parameters()]
    dev = m._arena.device
    for i in blks:
        for t in TARGETS:
            if t not in targets:
                continue
            mod, dotted, suffix = _site(m.blocks[i], t)
            w = mod._parameters["weight"]
            N = w.shape[0] // 3 if t in ("q", "k", "v") else w.shape[0]
            K = w.shape[1]
            bound = 1.0 / math.sqrt(K)
            a = torch.empty(rank, K, dtype=torch.float32).uniform_(-bound, bound, generator=generator)
            na, nb = "lora_A" + suffix, "lora_B" + suffix
            mod.register_parameter(na, nn.Parameter(a.to(dev)))
            mod.register_parameter(nb, nn.Parameter(torch.zeros(N, rank, dtype=torch.float32, device=dev)))
            lo.items.append((i, TARGETS.index(t), mod, na, nb, f"blocks.{i}.{dotted}."))
    if freeze_base:
        for p in m._arena_params:
            p.requires_grad_(False)
    m._lora = lo
    m._feat_cache = None
    return lo.params()


def lora_parameters(model):
    """The adapter parameters (A then B of every adapted Linear, blocks ascending); [] without adapters."""
    lo = getattr(_encoder(model), "_lora", None)
    return lo.params() if lo is not None else []


def lora_state_dict(model):
    """{key: detached clone} of the adapter tensors only."""
    return {k: p.detach().clone() for k, p in _state(model).named()}


def load_lora_state_dict(model, sd, strict=True):
    """Copy adapter tensors from `sd` (keys as lora_state_dict's) into the attached adapters; strict: a missing or unexpected key, and
    always a shape mismatch, is a RuntimeError.  Returns (missing, unexpected)."""
    named = dict(_state(model).named())
    missing = [k for k in named if k not in sd]
    unexpected = [k for k in sd if k not in named]
    if strict and (missing or unexpected):
        raise RuntimeError(f"load_lora_state_dict: missing keys {missing}, unexpected keys {unexpected}")
    for k, p in named.items():
        if k in sd and tuple(sd[k].shape) != tuple(p.shape):
            raise RuntimeError(f"load_lora_state_dict: {k} has shape {tuple(sd[k].shape)}, the adapter {tuple(p.shape)}")
    with torch.no_grad():
        for k, p in named.items():
            if k in sd:
                p.copy_(sd[k])
    model._feat_cache = None
    return missing, unexpected


def mark_only_lora_trainable(model, train_head=True):
    """requires_grad = False on every parameter of the model except the adapters (and the head's, with train_head)."""
    lo = _state(model)
    keep = {id(p) for p in lo.params()}
    if train_head and isinstance(model.head, nn.Module):
        keep |= {id(p) for p in model.head.parameters()}
    for p in model.parameters():
        p.requires_grad_(id(p) in keep)


def _detach(m, lo, restore_flags):
    for _, _, mod, na, nb, _ in lo.items:
        del mod._parameters[na], mod._parameters[nb]
    if restore_flags:
        live = {id(p) for p in m.parameters()}
        for p, flag in lo.base_flags:
            if id(p) in live:
                p.requires_grad_(flag)
    m._lora = None
    m._shadow_key = None        # the shadow holds merged weights: rebuilt from the arena on the next forward
    m._feat_cache = None


def merge_lora(model):
    """Fold s B A into the arena weights in place (mfvit_lora_merge with out == w: the arithmetic that built the effective weights, so
    the model's outputs afterwards are bit-identical to its outputs with the adapters attached), remove the adapter parameters and
    restore the state_dict() key set and the requires_grad flags from before add_lora."""
    m = _encoder(model)
    lo = _state(m)
    m.flat_parameters()         # (the holders' weights are views of the arena)
    with torch.no_grad():
        for _, code, mod, na, nb, _ in lo.items:
            w, a, b = mod._parameters["weight"], mod._parameters[na], mod._parameters[nb]
            N, K = b.shape[0], a.shape[1]
            rows = w.detach()[code * N:(code + 1) * N] if code <= 2 else w.detach()
            if rows.is_cuda:
                check(lib().mfvit_lora_merge(ptr(rows), K, ptr(a), ptr(b), lo.scale, ptr(rows), K, N, K, lo.rank, stream()), "mfvit_lora_merge")
            else:
                # a model that is not on the GPU holds no kernel state: the same sum in torch's f32 (j ascending is not promised here)
                rows.add_(lo.scale * (b.detach() @ a.detach()))
    _detach(m, lo, True)


def remove_lora(model):
    """Drop the adapters without folding them: the base model's bits come back (its arena was never written), with the state_dict() key
    set and the requires_grad flags from before add_lora."""
    m = _encoder(model)
    _detach(m, _state(m), True)
