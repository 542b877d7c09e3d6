"""ViT-S/16 backbone module backed by the gfx950 encoder kernels (libmfvit_hip.so).

Stands in for the module the reference imports as ``vits`` / ``vits_returnftrs`` (absent from its tree; SURVEY.md
§0.2, Appendix A): same constructor kwargs (``num_classes``, ``stop_grad_conv1``), same timm parameter names and
state-dict keys, ``.head`` a re-assignable ``nn.Linear``, ``forward(img) -> (B, num_classes)`` and
``features3D(img) -> (B, 1 + HW/256, 384)``.

timm's regularisation kwargs (``drop_rate``, ``attn_drop_rate``, ``drop_path_rate``; moco-v3 ``vits.py`` passes them on) are honoured in
training mode: parameter-free ``pos_drop`` / ``attn.attn_drop`` / ``attn.proj_drop`` / ``mlp.drop`` / ``blocks[i].drop_path`` modules carry
the rates, and every training-mode forward draws fresh masks (include/mfvit.h, mfvit_vit_drop) from a seed taken from torch's CPU generator.

MI355X-first layout: every backbone parameter is a view into ONE flat f32 arena (timm registration order, the
layout of include/mfvit.h), so the encoder kernels, the fused optimizers, the EMA update and the gradient
all-reduce all work on contiguous slices.  Gradients come back from the C ABI as one flat arena as well.
There is no CPU / eager fallback: forward on a non-GPU tensor raises.
"""
import contextlib
import ctypes
import math
import operator
import os

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import VitCfg, check, lib, ptr, stream


def default_precision():
    """'bf16x3' (split bf16: f32-grade results on the bf16 matrix core) unless MFVIT_PRECISION says otherwise: the reference's
    finetune paths are fp32 (no autocast in MAIN_CA / MAIN_SS), so the default must meet the 1e-3 logits gate.  'bf16' is the
    throughput mode, 'fp16' the reference's autocast pretraining arithmetic (MAIN_MOCO:349), 'fp32' exact f32 MFMA."""
    return os.environ.get("MFVIT_PRECISION", "bf16x3")


def build_2d_sincos_position_embedding(gh, gw, dim, temperature=10000.0):
    """Fixed 2-D sin-cos table with a zero cls slot (moco-v3 ``vits.py``).  float64 -> float32."""
    assert dim % 4 == 0, "embed dim must be divisible by 4 for the 2-D sin-cos position embedding"
    gw_, gh_ = torch.meshgrid(torch.arange(gw, dtype=torch.float64), torch.arange(gh, dtype=torch.float64), indexing="ij")
    pos_dim = dim // 4
    omega = 1.0 / (temperature ** (torch.arange(pos_dim, dtype=torch.float64) / pos_dim))
    out_w = gw_.flatten()[:, None] * omega[None]
    out_h = gh_.flatten()[:, None] * omega[None]
    pe = torch.cat([out_w.sin(), out_w.cos(), out_h.sin(), out_h.cos()], dim=1)[None]
    return torch.cat([torch.zeros(1, 1, dim, dtype=torch.float64), pe], dim=1).float()


def check_target(target, B, C):
    """The target class of a relevance call as a (B,) int64 CPU tensor (None stays None: the argmax of the model's output), or ValueError for
    a bad type, shape or class - before anything is launched.  C: the number of classes (None: not known before the head has run; the
    upper bound is then checked by resolve_target)."""
    if target is None:
        return None
    if isinstance(target, torch.Tensor):
        if target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
            raise ValueError(f"target must hold integer classes, got dtype {target.dtype}")
        if tuple(target.shape) != (B,):
            raise ValueError(f"target tensor must have shape ({B},), got {tuple(target.shape)}")
        t = target.detach().to("cpu", torch.int64)
    else:
        try:
            if isinstance(target, bool):
                raise TypeError
            t = torch.full((B,), operator.index(target), dtype=torch.int64)
        except TypeError:
            raise ValueError(f"target must be None, an int or a ({B},) integer tensor, got {target!r}") from None
    if B and (int(t.min()) < 0 or (C is not None and int(t.max()) >= C)):
        raise ValueError(f"target class out of range for {C} classes: {t.tolist()}")
    return t


def resolve_target(target, out):
    """The (B, 1) device index of the scored class: the checked target, or the argmax of out (B, C)."""
    if target is None:
        return out.detach().argmax(dim=1, keepdim=True)
    if target.numel() and int(target.max()) >= out.shape[1]:
        raise ValueError(f"target class out of range for {out.shape[1]} classes: {target.tolist()}")
    return target.to(out.device).view(-1, 1)


@contextlib.contextmanager
def eval_modules(*mods):
    """Every module under mods in evaluation mode for the block (no BatchNorm statistic moves, no dropout); training flags restored after,
    also on error."""
    saved = [(m, m.training) for mod in mods if mod is not None for m in mod.modules()]
    try:
        for m, _ in saved:
            m.training = False
        yield
    finally:
        for m, t in saved:
            m.training = t


class _WB(nn.Module):
    """Parameter holder with timm-compatible child names (``weight`` / ``bias``)."""

    def __init__(self, w_shape, b_shape=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*w_shape))
        self.bias = nn.Parameter(torch.empty(*b_shape)) if b_shape is not None else None


class _Attn(nn.Module):
    def __init__(self, dim, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.qkv = _WB((3 * dim, dim), (3 * dim,))
        self.attn_drop = nn.Dropout(attn_drop)       # (rate carriers: parameter-free, the kernels apply them)
        self.proj = _WB((dim, dim), (dim,))
        self.proj_drop = nn.Dropout(proj_drop)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden, drop=0.0):
        super().__init__()
        self.fc1 = _WB((hidden, dim), (hidden,))
        self.fc2 = _WB((dim, hidden), (dim,))
        self.drop = nn.Dropout(drop)                 # timm Mlp: after the GELU and after fc2


class _Block(nn.Module):
    def __init__(self, dim, hidden, drop=0.0, attn_drop=0.0, drop_path=0.0):
        super().__init__()
        self.norm1 = _WB((dim,), (dim,))
        self.attn = _Attn(dim, attn_drop, drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()     # (timm 0.4.9)
        self.norm2 = _WB((dim,), (dim,))
        self.mlp = _Mlp(dim, hidden, drop)


class DropPath(nn.Module):
    """Rate carrier of timm's per-sample stochastic depth (``drop_prob``): the encoder kernels apply it, this module is never called."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def extra_repr(self):
        return f"drop_prob={self.drop_prob}"


class PatchDropout(nn.Module):
    """Rate carrier of timm >= 0.9 ``PatchDropout(prob, num_prefix_tokens=1, ordered=False)`` (Liu et al. 2022; FLIP): in training mode the blocks
    run on cls and ``K = max(1, int(L * (1 - prob)))`` of the L patch rows per image.  The encoder's front end (csrc/patch_drop.hip) applies it,
    this module is never called."""

    def __init__(self, prob=0.0, num_prefix_tokens=1, ordered=False):
        super().__init__()
        self.prob = float(prob)
        self.num_prefix_tokens = int(num_prefix_tokens)
        self.ordered = bool(ordered)

    def num_keep(self, L):
        return max(1, int(L * (1.0 - self.prob)))

    def draw(self, B, L, device):
        """(B, K) int64 indices of the kept patches, timm's draw: argsort of a normal sample per image, from torch's generator of `device`."""
        idx = torch.argsort(torch.randn(B, L, device=device), dim=-1)[:, :self.num_keep(L)]
        if self.ordered:
            idx = idx.sort(dim=-1)[0]
        return idx.contiguous()

    def extra_repr(self):
        return f"prob={self.prob}, num_prefix_tokens={self.num_prefix_tokens}, ordered={self.ordered}"


class _PatchEmbed(nn.Module):
    def __init__(self, dim, patch):
        super().__init__()
        self.proj = _WB((dim, 3, patch, patch), (dim,))


class _EncoderFn(torch.autograd.Function):
    """features3D as one autograd node.  forward: the chain of VisionTransformerMoCo._forward_chain - the patch-dropout front end on the kept
    patches `idx` (None: the image goes to the first range), then the block ranges of _token_segments with score / select / reorganise between
    two of them (one range [0, depth) without token pruning; `forced`: checked selections or None).  backward: the same chain in reverse, stage
    group by stage group (_backward_chain); d loss / d img when the image requires a gradient, and no parameter gradient at all when no arena
    parameter requires one.  The kept patches, the selections and the fused row's weights are constants: no gradient flows to them.
    params: the arena parameters, then the adapter parameters of mfvit.lora (if attached); with adapters and every arena parameter frozen the
    backward is mfvit_vit_backward_lora (the data-gradient chain + the adapted Linears' weight gradients)."""

    @staticmethod
    def forward(ctx, model, img, idx, forced, need_grad, drop, *params):
        # drop: the mfvit_vit_drop of THIS forward (None: no dropout site active)
        want_dimg = bool(need_grad and ctx.needs_input_grad[1])
        plan = model._token_segments(model.num_tokens if idx is None else idx.shape[1] + 1)
        feats, state = model._forward_chain(img, idx, plan, forced, need_grad, drop, want_dimg)
        ctx.model = model
        ctx.state = state
        ctx.cfg = model._cfg(img, need_grad)
        ctx.drop = drop                     # the backward rebuilds the same masks from it
        ctx.want_dimg = want_dimg
        ctx.img_meta = (img.shape, img.dtype)
        return feats

    @staticmethod
    def backward(ctx, dfeats):
        model = ctx.model
        if torch.is_grad_enabled():
            raise _lib.MfvitError("double backward through the encoder (create_graph=True) is not supported: its backward is one HIP call "
                                  "whose results are not differentiable")
        if ctx.state is None:
            raise _lib.MfvitError("the encoder's saved activations were already released: a second backward through the same forward "
                                  "(retain_graph=True) is not supported - run the forward again")
        dimg = None
        if ctx.want_dimg and ctx.needs_input_grad[1]:
            shape, dtype = ctx.img_meta
            # (allocated on the current stream - the side stream of a two-stream model's ENH encoder - and recorded there: autograd hands it
            # to consumers on other streams)
            dimg = torch.empty(shape, device=dfeats.device, dtype=torch.float32)
            dimg.record_stream(torch.cuda.current_stream(dfeats.device))
        na = len(model._arena_params)
        need = ctx.needs_input_grad[6:]
        want_params, want_lora = any(need[:na]), any(need[na:])
        if want_lora and not want_params:       # (adapters run on the full grid only: one range, its workspace)
            grads = [None] * na + model._run_backward_lora(ctx.cfg, ctx.state[0][0][1], dfeats, drop=ctx.drop, dimg=dimg)
        else:
            grads = model._backward_chain(ctx.cfg, ctx.state, dfeats, drop=ctx.drop, dimg=dimg, want_params=want_params)
            if want_lora:       # adapters beside trainable arena parameters: contract the adapted dW slices of the full gradient arena
                grads = grads + model._lora_grads_from_arena(ctx.cfg, model._last_grad_arena)
            else:
                grads = grads + [None] * (len(need) - na)
        grads = [g if n else None for g, n in zip(grads, need)]
        model._release_state(ctx.state)
        ctx.state = None
        # the single-use feature cache holds the forward's output, i.e. this graph and the parameters' AccumulateGrad nodes (which carry
        # the stream they were created under): once the backward has run it must not keep them alive into the next iteration
        model._feat_cache = None
        if dimg is not None and dimg.dtype != ctx.img_meta[1]:
            dimg = dimg.to(ctx.img_meta[1])
        return (None, dimg, None, None, None, None) + tuple(grads)


class _HeadFn(torch.autograd.Function):
    """Small classifier head on the cls rows of a token tensor: y = feats[:, 0] @ W.T + b (f32)."""

    @staticmethod
    def forward(ctx, feats, w, b):
        B, T, D = feats.shape
        feats = feats if feats.is_contiguous() else feats.contiguous()
        y = ops.head_fwd(feats, w, b, ldx=T * D)
        ctx.save_for_backward(feats, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        feats, w = ctx.saved_tensors
        B, T, D = feats.shape
        dy = dy.contiguous()
        dfe = dw = db = None
        if ctx.needs_input_grad[0]:
            dfe = torch.zeros_like(feats)
        if ctx.needs_input_grad[1]:
            dw = torch.zeros_like(w)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = torch.zeros(w.shape[0], device=w.device, dtype=torch.float32)
        ops.head_bwd(dy, feats, w, ldx=T * D, dx=dfe, lddx=T * D, dw=dw, db=db)
        return dfe, dw, db


class VisionTransformerMoCo(nn.Module):
    def __init__(self, img_size=224, patch_size=16, embed_dim=384, depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True,
                 num_classes=1000, stop_grad_conv1=False, precision=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 patch_drop_rate=0.0, patch_drop_ordered=False, token_keep_rate=1.0, token_prune_blocks=None, token_fuse=True,
                 **unused_timm_kwargs):
        super().__init__()
        for name, r in (("drop_rate", drop_rate), ("attn_drop_rate", attn_drop_rate), ("drop_path_rate", drop_path_rate),
                        ("patch_drop_rate", patch_drop_rate)):
            if not 0.0 <= float(r) < 1.0:
                raise ValueError(f"{name} must lie in [0, 1), got {r!r}")
        if patch_size != 16:
            raise NotImplementedError("only patch_size=16 (ViT-S/16) is built")
        if embed_dim not in (384, 768):
            raise NotImplementedError("the gfx950 encoder is built for embed_dim 384 (vit_small: row-complete GEMM kernels with fused LayerNorm "
                                      "epilogues) and 768 (vit_base: tile GEMMs + LayerNorm row passes)")
        if not qkv_bias:
            raise NotImplementedError("qkv_bias=False is not used by the reference (moco-v3 vits: qkv_bias=True)")
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        self.embed_dim = self.num_features = embed_dim
        self.depth = depth
        self.num_heads = num_heads
        self.mlp_dim = int(embed_dim * mlp_ratio)
        self.num_classes = num_classes
        self.stop_grad_conv1 = bool(stop_grad_conv1)
        self.precision = precision or default_precision()
        _lib.dtype_code(self.precision)  # validate
        gh, gw = self.img_size[0] // 16, self.img_size[1] // 16
        self.num_tokens = gh * gw + 1

        # ---- parameters, timm registration order (== arena order)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(build_2d_sincos_position_embedding(gh, gw, embed_dim), requires_grad=False)
        self.patch_embed = _PatchEmbed(embed_dim, 16)
        self.pos_drop = nn.Dropout(float(drop_rate))
        self.patch_drop = PatchDropout(float(patch_drop_rate), 1, bool(patch_drop_ordered))     # (timm: between pos_drop and the blocks)
        dpr = [x.item() for x in torch.linspace(0, float(drop_path_rate), depth)]       # stochastic depth decay rule (timm)
        self.blocks = nn.ModuleList([_Block(embed_dim, self.mlp_dim, float(drop_rate), float(attn_drop_rate), dpr[i]) for i in range(depth)])
        self.norm = _WB((embed_dim,), (embed_dim,))
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        self._init_weights()
        if self.stop_grad_conv1:
            self.patch_embed.proj.weight.requires_grad = False
            self.patch_embed.proj.bias.requires_grad = False

        self._arena = None
        self._shadow = None
        self._shadow_key = None
        self._ws_pool = {}
        self._feat_cache = None
        self._lora = None                   # mfvit.lora.LoraState while adapters are attached
        self.last_keep_indices = None       # (B, K) int64: the kept patches of the last training-mode forward under patch dropout
        # token pruning between blocks (EViT; csrc/token_prune.hip): plain attributes, read on every forward - the rate may change between steps
        self.token_keep_rate = float(token_keep_rate)
        self.token_prune_blocks = (tuple(sorted({l for l in (depth // 4, depth // 2, 3 * depth // 4) if 0 <= l <= depth - 2}))
                                   if token_prune_blocks is None else tuple(token_prune_blocks))
        self.token_fuse = bool(token_fuse)
        self._token_plan()                  # (validates)
        self.last_token_indices = None      # [(B, K) int64 per executed stage, in that stage's own row numbering] of the last pruned forward
        self._last_token_plan = None        # (T0, fuse) of that forward: what token_origin() composes with
        self._prune_sizes = {}              # workspace sizes of the current token plan, per kind of call (_retain_prune_sizes)
        self._keep_pin = None               # a draw pinned by the model that drives this encoder (Fus_CrossViT: one draw per step)
        self._keep_err = None               # the front end's device error word (a patch index outside the grid)
        self._flatten()

    # ------------------------------------------------------------------ init (moco-v3 VisionTransformerMoCo)
    def _init_weights(self):
        D = self.embed_dim
        with torch.no_grad():
            nn.init.normal_(self.cls_token, std=1e-6)
            val = math.sqrt(6.0 / float(3 * 16 * 16 + D))
            nn.init.uniform_(self.patch_embed.proj.weight, -val, val)
            nn.init.zeros_(self.patch_embed.proj.bias)
            for blk in self.blocks:
                nn.init.ones_(blk.norm1.weight); nn.init.zeros_(blk.norm1.bias)
                nn.init.ones_(blk.norm2.weight); nn.init.zeros_(blk.norm2.bias)
                v = math.sqrt(6.0 / float(blk.attn.qkv.weight.shape[0] // 3 + blk.attn.qkv.weight.shape[1]))
                nn.init.uniform_(blk.attn.qkv.weight, -v, v)      # q, k, v treated as separate matrices
                nn.init.zeros_(blk.attn.qkv.bias)
                for m in (blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                    nn.init.xavier_uniform_(m.weight)
                    nn.init.zeros_(m.bias)
            nn.init.ones_(self.norm.weight); nn.init.zeros_(self.norm.bias)
            if isinstance(self.head, nn.Linear):
                nn.init.xavier_uniform_(self.head.weight)
                nn.init.zeros_(self.head.bias)

    # ------------------------------------------------------------------ flat arena
    def _param_holders(self):
        """(name, holder module, attribute) of every arena parameter in arena order (include/mfvit.h); built once - the module tree of the
        encoder is fixed at construction.  The parameters themselves are looked up through the holders on every use (a caller may rebind
        ``holder.weight``), without going through ``nn.Module.__getattr__`` and without formatting 150 names per call (host time of a
        small-batch step, tools/host_profile.py)."""
        h = self.__dict__.get("_holders")
        if h is None:
            pe = self.patch_embed.proj
            h = [("cls_token", self, "cls_token"), ("pos_embed", self, "pos_embed"),
                 ("patch_embed.proj.weight", pe, "weight"), ("patch_embed.proj.bias", pe, "bias")]
            for i, b in enumerate(self.blocks):
                p = f"blocks.{i}."
                for mod_name, mod in (("norm1", b.norm1), ("attn.qkv", b.attn.qkv), ("attn.proj", b.attn.proj), ("norm2", b.norm2),
                                      ("mlp.fc1", b.mlp.fc1), ("mlp.fc2", b.mlp.fc2)):
                    h += [(p + mod_name + ".weight", mod, "weight"), (p + mod_name + ".bias", mod, "bias")]
            h += [("norm.weight", self.norm, "weight"), ("norm.bias", self.norm, "bias")]
            self.__dict__["_holders"] = h
        return h

    def arena_named_parameters(self):
        """(name, Parameter) in arena order (include/mfvit.h); the classifier head is not part of the arena."""
        return [(name, mod._parameters[attr]) for name, mod, attr in self._param_holders()]

    def _flatten(self):
        named = self.arena_named_parameters()
        total = sum(p.numel() for _, p in named)
        dev = named[0][1].device
        arena = torch.empty(total, device=dev, dtype=torch.float32)
        off = 0
        self._offsets = {}
        with torch.no_grad():
            for name, p in named:
                n = p.numel()
                arena[off:off + n].copy_(p.data.reshape(-1).float())
                p.data = arena[off:off + n].view(p.shape)
                self._offsets[name] = (off, n)
                off += n
        self._arena = arena
        self._arena_params = [p for _, p in named]
        self._arena_offsets = [self._offsets[name][0] for name, _ in named]      # (same order as _param_holders())
        self._shadow = None
        self._shadow_key = None
        self._ws_pool = {}
        self._prune_sizes = {}
        self._feat_cache = None

    def _arena_intact(self):
        base = self._arena.data_ptr()
        f32 = torch.float32
        for (_, mod, attr), off in zip(self._param_holders(), self._arena_offsets):
            p = mod._parameters[attr]
            if p.data_ptr() != base + 4 * off or p.dtype != f32:
                return False
        return True

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._flatten()  # parameters were moved / cast one by one: rebuild the arena on the new device
        return out

    def flat_parameters(self):
        """The flat f32 arena holding every backbone parameter (head excluded)."""
        if not self._arena_intact():
            self._flatten()
        return self._arena

    def arena_slice(self, name):
        return self._offsets[name]

    def block_slice(self, i):
        """(offset, length) of block i in the arena / gradient arena (one all-reduce bucket)."""
        a = self._offsets[f"blocks.{i}.norm1.weight"][0]
        o, n = self._offsets[f"blocks.{i}.mlp.fc2.bias"]
        return a, o + n - a

    # ------------------------------------------------------------------ training-mode dropout
    def drop_rates(self):
        """(drop_rate, attn_drop_rate, [drop-path rate of every block]) as the rate-carrier modules hold them now."""
        # (read on every training-mode forward: plain `_modules` lookups, not nn.Module.__getattr__ - host time of a small-batch step)
        blocks = list(self._modules["blocks"]._modules.values())
        drop = float(self._modules["pos_drop"].p)
        attn = float(blocks[0]._modules["attn"]._modules["attn_drop"].p)
        dpr = []
        for b in blocks:
            a, mlp = b._modules["attn"]._modules, b._modules["mlp"]._modules
            if float(a["proj_drop"].p) != drop or float(mlp["drop"].p) != drop or float(a["attn_drop"].p) != attn:
                raise _lib.MfvitError("the encoder kernels take one drop_rate (pos_drop, proj_drop, mlp.drop) and one attn_drop_rate for all "
                                      "blocks: set the rate-carrier modules consistently")
            dpr.append(float(getattr(b._modules["drop_path"], "drop_prob", 0.0)))
        for r in [drop, attn] + dpr:
            if not 0.0 <= r < 1.0:
                raise _lib.MfvitError(f"dropout rates must lie in [0, 1), got {r}")
        return drop, attn, dpr

    def is_stochastic(self):
        """True in training mode with any dropout / drop-path rate > 0: every forward then draws masks of its own."""
        if not self.training:
            return False
        drop, attn, dpr = self.drop_rates()
        if drop > 0.0 or attn > 0.0 or any(r > 0.0 for r in dpr):
            return True
        # patch dropout: a forward of its own per call, unless the driving model has pinned one draw for the step
        return self._patch_drop_prob() > 0.0 and self.__dict__.get("_keep_pin") is None

    # ------------------------------------------------------------------ patch dropout (timm PatchDropout; csrc/patch_drop.hip)
    def _patch_drop_prob(self):
        pd = self._modules.get("patch_drop")
        p = float(getattr(pd, "prob", 0.0))
        if not 0.0 <= p < 1.0:
            raise _lib.MfvitError(f"patch_drop.prob must lie in [0, 1), got {p}")
        return p

    def draw_keep_indices(self, B, device=None):
        """The (B, K) int64 kept-patch indices of one training-mode forward as timm's PatchDropout draws them (argsort of randn on the model's
        device, from torch's generator: `torch.manual_seed` reproduces them), or None in eval() / at rate 0."""
        if not self.training or self._patch_drop_prob() <= 0.0:
            return None
        return self.patch_drop.draw(int(B), self.num_tokens - 1, device if device is not None else self._arena.device)

    @contextlib.contextmanager
    def pinned_keep_indices(self, idx):
        """Every forward inside the block keeps the patches `idx` ((B, K) int64 on the model's device, distinct and in range - not checked
        again; None: nothing pinned): features3D and the head forward of one step then share one draw and the single-use feature cache holds."""
        prev = self.__dict__.get("_keep_pin")
        self._keep_pin = idx
        try:
            yield
        finally:
            self._keep_pin = prev

    def _check_keep_indices(self, idx, B):
        """Explicit indices, checked on the host (one sync): (B, K) integers, 1 <= K <= L, in [0, L), distinct per image."""
        L = self.num_tokens - 1
        if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype.is_floating_point or idx.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise _lib.MfvitError("keep_indices must be a (B, K) integer tensor")
        if idx.shape[0] != B or not 1 <= idx.shape[1] <= L:
            raise _lib.MfvitError(f"keep_indices must have shape ({B}, K) with 1 <= K <= {L}, got {tuple(idx.shape)}")
        idx = idx.detach().to(self._arena.device, torch.int64).contiguous()
        srt = idx.sort(dim=-1)[0]
        bad_range = (srt[:, 0] < 0).any() | (srt[:, -1] >= L).any()
        dup = (srt[:, 1:] == srt[:, :-1]).any() if idx.shape[1] > 1 else torch.zeros((), dtype=torch.bool, device=idx.device)
        flags = torch.stack([bad_range, dup]).tolist()
        if flags[0]:
            raise _lib.MfvitError(f"keep_indices out of range for {L} patches")
        if flags[1]:
            raise _lib.MfvitError("keep_indices repeat a patch within an image")
        self.check_keep_error()
        return idx

    def check_keep_error(self):
        """Raises MfvitError when a front-end kernel met a patch index outside the grid since the last check (such a row is zeros and never
        becomes an address).  Reads the device error word: one sync.  Called by every forward with explicit indices; call it yourself after
        forwards that pin or draw indices of your own making."""
        e = self._keep_err
        if e is not None and int(e.item()) != 0:
            e.zero_()
            raise _lib.MfvitError("patch dropout: a kept-patch index outside the grid reached the device (its row was dropped)")

    def _resolve_keep(self, x, keep_indices):
        """The (B, K) indices this forward keeps, or None: the full sequence."""
        if keep_indices is not None and not self.training:
            raise _lib.MfvitError("keep_indices is a training-mode argument: eval() runs every patch (timm PatchDropout)")
        pin = self.__dict__.get("_keep_pin") if self.training else None
        active = keep_indices is not None or pin is not None or (self.training and self._patch_drop_prob() > 0.0)
        if active and self.__dict__.get("_lora") is not None:       # (before anything is drawn or checked on the device)
            raise _lib.MfvitError("LoRA adapters together with an active patch dropout are not built: the shortened sequence runs on the plain "
                                  "parameter arena (set patch_drop.prob = 0, or detach the adapters)")
        if keep_indices is not None:
            return self._check_keep_indices(keep_indices, int(x.shape[0]))
        return pin if pin is not None else self.draw_keep_indices(x.shape[0], x.device)

    # ------------------------------------------------------------------ token pruning between blocks (EViT; csrc/token_prune.hip)
    def _token_plan(self):
        """(keep_rate, prune_blocks, fuse) as the attributes hold them now, checked; prune_blocks () when nothing is pruned."""
        rate = float(self.token_keep_rate)
        if not 0.0 < rate <= 1.0:
            raise _lib.MfvitError(f"token_keep_rate must lie in (0, 1], got {self.token_keep_rate!r}")
        try:
            blocks = tuple(operator.index(l) for l in self.token_prune_blocks)
        except TypeError:
            raise _lib.MfvitError(f"token_prune_blocks must hold block indices, got {self.token_prune_blocks!r}") from None
        if any(not 0 <= l <= self.depth - 2 for l in blocks) or any(a >= b for a, b in zip(blocks, blocks[1:])):
            raise _lib.MfvitError(f"token_prune_blocks must be strictly increasing block indices in [0, {self.depth - 2}], got {blocks}")
        return rate, (blocks if rate < 1.0 else ()), bool(self.token_fuse)

    def token_pruning_active(self):
        """True when a forward would shorten the sequence between blocks (token_keep_rate < 1 and a prune block)."""
        rate, blocks, _ = self._token_plan()
        return rate < 1.0 and len(blocks) > 0

    @staticmethod
    def _token_keep(T, rate):
        return max(1, min(T - 1, int(math.ceil(rate * (T - 1)))))

    def _token_segments(self, T):
        """[(block_lo, block_hi, tokens)] of a forward that starts with T rows per image: a new segment behind every prune block whose
        stage is not skipped (K == T - 1 keeps the sequence)."""
        rate, blocks, fuse = self._token_plan()
        segs, lo = [], 0
        for l in blocks:
            K = self._token_keep(T, rate)
            if K < T - 1:
                segs.append((lo, l + 1, T))
                lo, T = l + 1, 1 + K + int(fuse)
        return segs + [(lo, self.depth, T)]

    def token_schedule(self, T=None):
        """Tokens per image of every segment of a forward that starts with T rows (default: the full grid, cls included).  Host only."""
        T = self.num_tokens if T is None else operator.index(T)
        if not 2 <= T <= self.num_tokens:
            raise _lib.MfvitError(f"T must lie in [2, {self.num_tokens}], got {T}")
        return [t for _, _, t in self._token_segments(T)]

    def token_origin(self):
        """(B, T_last - 1) int64: the row (cls not counted) of the sequence in front of block 0 that every non-cls row of the last pruned forward's
        output came from, -1 for a fused row.  Under patch dropout these are positions in last_keep_indices."""
        sel = self.last_token_indices
        if not sel:
            raise _lib.MfvitError("no pruned forward has run")
        B = sel[0].shape[0]
        T0, fuse = self._last_token_plan
        org = torch.arange(T0 - 1, device=sel[0].device).expand(B, -1)
        for keep in sel:
            org = torch.gather(org, 1, keep)
            if fuse:
                org = torch.cat([org, org.new_full((B, 1), -1)], dim=1)
        return org

    def _refuse_if_pruning(self, what):
        if self.token_pruning_active():
            raise _lib.MfvitError(f"{what} assumes the full token grid and is not built for an encoder that prunes tokens between blocks: set "
                                  "token_keep_rate = 1.0 for this call")

    def _check_token_indices(self, token_indices, B, T0):
        """Forced selections, checked on the host (one sync): one (B, K) integer tensor per stage of the schedule, each in that stage's own row
        numbering, in range and distinct per image.  Returns them as ascending int32 device tensors."""
        segs = self._token_segments(T0)
        if not isinstance(token_indices, (list, tuple)) or len(token_indices) != len(segs) - 1:
            raise _lib.MfvitError(f"token_indices must be a list of {len(segs) - 1} (B, K) integer tensors, one per pruning stage")
        out, flags = [], []
        for (_, _, T), (_, _, Tn), idx in zip(segs, segs[1:], token_indices):
            K = Tn - 1 - int(self.token_fuse)
            if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype.is_floating_point or idx.dtype in (torch.bool, torch.complex64,
                                                                                                                 torch.complex128):
                raise _lib.MfvitError("token_indices must hold (B, K) integer tensors")
            if tuple(idx.shape) != (B, K):
                raise _lib.MfvitError(f"token_indices of the stage on {T} rows must have shape ({B}, {K}), got {tuple(idx.shape)}")
            srt = idx.detach().to(self._arena.device, torch.int64).sort(dim=-1)[0]
            flags.append((srt[:, 0] < 0).any() | (srt[:, -1] >= T - 1).any())
            flags.append((srt[:, 1:] == srt[:, :-1]).any() if K > 1 else torch.zeros((), dtype=torch.bool, device=srt.device))
            out.append(srt.to(torch.int32).contiguous())
        if flags and any(torch.stack(flags).tolist()):
            raise _lib.MfvitError("token_indices out of range for their stage, or repeating a row within an image")
        self.check_keep_error()
        return out

    def _draw_drop(self):
        """mfvit_vit_drop of one training-mode forward (None when no site is active: eval(), or all rates 0).  The seed comes from torch's CPU
        generator, so `torch.manual_seed` makes the masks reproducible (as model/fuseattention.py does for the GPT).  One walk over the rate
        carriers per forward, none in eval()."""
        if not self.training:
            return None
        drop, attn, dpr = self.drop_rates()
        if not (drop > 0.0 or attn > 0.0 or any(r > 0.0 for r in dpr)):
            return None
        if _lib.dtype_code(self.precision) == _lib.F32:
            raise _lib.MfvitError("dropout / drop path inside the encoder is built for precision 'bf16x3' (f32-grade), 'bf16' and 'fp16', not 'fp32': "
                                  "use one of those, or train with the rates at 0")
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        rates = (ctypes.c_float * len(dpr))(*dpr)
        d = _lib.VitDrop(drop, attn, ctypes.cast(rates, ctypes.POINTER(ctypes.c_float)), seed)
        d._rates = rates                    # (keeps the host array alive as long as the struct)
        self._last_drop = d                 # (tests: the seed of the last training-mode forward, to export its masks)
        return d

    # ------------------------------------------------------------------ engine plumbing
    def _cfg(self, img, save):
        c = VitCfg()
        c.dtype = _lib.dtype_code(self.precision)
        c.batch, _, c.img_h, c.img_w = img.shape
        c.dim, c.depth, c.heads, c.mlp_dim = self.embed_dim, self.depth, self.num_heads, self.mlp_dim
        c.save_for_backward = int(bool(save))
        c.stop_grad_conv1 = int(not self.patch_embed.proj.weight.requires_grad)
        c.ln_eps = 1e-6
        c.stream_share = int(getattr(self, "_stream_share", 0))     # launch-geometry hint of the model that drives this encoder (0: the library default)
        return c

    def _param_version(self):
        v = sum(p._version for p in self._arena_params)
        lo = self.__dict__.get("_lora")
        # with adapters (mfvit.lora): their versions and the attachment's serial number are part of every key the weights enter -
        # the shadow's and the single-use feature cache's
        return v if lo is None else (v, lo.serial, sum(p._version for p in lo.params()))

    def _kernel_params(self):
        """The f32 arena the encoder entry points take as `params`: the parameter arena, or with adapters the effective arena
        (every adapted weight merged, W + s B A) that _ensure_shadow keeps beside the shadow."""
        lo = self.__dict__.get("_lora")
        return self._arena if lo is None else lo.eff

    def _ensure_shadow(self, cfg):
        key = (self._param_version(), cfg.dtype, str(self._arena.device))
        if self._shadow is not None and key == self._shadow_key:
            return
        if not self._arena_intact():
            self._flatten()
            key = (self._param_version(), cfg.dtype, str(self._arena.device))
        nbytes = lib().mfvit_vit_shadow_bytes(cfg)
        if self._shadow is None or self._shadow.numel() != nbytes:
            self._shadow = torch.empty(nbytes, device=self._arena.device, dtype=torch.uint8)
        lo = self.__dict__.get("_lora")
        if lo is None:
            check(lib().mfvit_vit_prepare_shadow(cfg, ptr(self._arena), ptr(self._shadow), stream()), "mfvit_vit_prepare_shadow")
        else:
            # the shadow of the merged weights; the effective arena is what forward and backward read as `params`
            if lo.eff is None or lo.eff.shape != self._arena.shape or lo.eff.device != self._arena.device:
                lo.eff = torch.empty_like(self._arena)
            req = lo.request(grads=None)
            check(lib().mfvit_vit_prepare_shadow_lora(cfg, ptr(self._arena), req, ptr(lo.eff), ptr(self._shadow), stream()),
                  "mfvit_vit_prepare_shadow_lora")
        self._shadow_key = key
        self._feat_cache = None

    def _take_ws(self, nbytes, dev):
        """A workspace of nbytes from the pool, or a new one."""
        pool = self._ws_pool.setdefault(nbytes, [])
        return pool.pop() if pool else torch.empty(nbytes, device=dev, dtype=torch.uint8)

    def _get_ws(self, cfg, drop=None, want_dimg=False):
        """A full-grid workspace (want_dimg: the image gradient's W_pe^T behind the usual layout: include/mfvit.h, mfvit_vit_workspace_bytes_ex)."""
        nbytes = lib().mfvit_vit_workspace_bytes_ex(cfg, drop, int(bool(want_dimg)))
        if nbytes == 0:
            raise _lib.MfvitError("invalid encoder configuration (image size must be a multiple of 16, dim 384 or 768, head_dim 32 / 64 / 96)")
        return self._take_ws(nbytes, self._arena.device)

    def _release_ws(self, ws):
        if ws is not None:
            pool = self._ws_pool.setdefault(ws.numel(), [])
            if len(pool) < 2:
                pool.append(ws)

    # The workspaces of the block ranges are sized by the token plan, and token_keep_rate may change from step to step (EViT warms it up): the
    # pool keeps the sizes of the CURRENT plan of every kind of call (saving or not, with d img, with dropout, batch size, patch dropout in
    # front) and lets every other range workspace go - a warm-up through sixty rates holds one plan's buffers, not sixty.
    def _retain_prune_sizes(self, kind, sizes):
        new = frozenset(sizes)
        old = self._prune_sizes.get(kind)
        self._prune_sizes[kind] = new
        if old is not None and old != new:
            live = frozenset().union(*self._prune_sizes.values())
            for n in old - live:
                self._ws_pool.pop(n, None)

    def _release_prune_ws(self, ws):
        if ws is not None and any(ws.numel() in s for s in self._prune_sizes.values()):
            self._release_ws(ws)

    def _release_state(self, state):
        """The workspaces of a forward's state back to the pool: the ranges' by the policy they were taken under, the front end's."""
        ranges, _, front, _, pruning = state
        for _, ws in ranges:
            (self._release_prune_ws if pruning else self._release_ws)(ws)
        if front is not None:
            self._release_ws(front[2])

    def _prep_img(self, img):
        """The image as the encoder entry points take it (contiguous f32 NCHW on the model's device), or MfvitError."""
        _lib.require_cuda(img)
        if img.dtype != torch.float32:
            img = img.float()
        img = img.contiguous()
        if img.shape[1] != 3 or (img.shape[2], img.shape[3]) != self.img_size:
            raise _lib.MfvitError(f"expected (B,3,{self.img_size[0]},{self.img_size[1]}) images, got {tuple(img.shape)} "
                                  "(pos_embed is size-bound)")
        if self._arena.device != img.device:
            raise _lib.MfvitError(f"model on {self._arena.device} but input on {img.device}")
        return img

    def _keep_embed(self, cfg, img, idx, save):
        """The patch-dropout front end (csrc/patch_drop.hip): (x0 (B, 1 + K, D), front) with front = (tokens, mfvit_patch_keep_cfg, the front
        end's workspace or None without save, idx) for _keep_embed_bwd."""
        dev = img.device
        if idx.device != dev:
            raise _lib.MfvitError(f"keep indices on {idx.device} but input on {dev}")
        idx.record_stream(torch.cuda.current_stream(dev))     # (a step's draw is made on the caller's stream and may run on the side stream)
        B, K = idx.shape
        pk = _lib.PatchKeepCfg(cfg.dtype, B, cfg.img_h, cfg.img_w, K, self.embed_dim)
        fbytes = lib().mfvit_patch_keep_workspace_bytes(pk, int(bool(save)))
        if fbytes == 0:
            raise _lib.MfvitError(f"invalid encoder configuration for patch dropout (image size a multiple of 16, dim 384 or 768, 1 <= K <= "
                                  f"{self.num_tokens - 1})")
        fws = self._take_ws(fbytes, dev)
        a, off = self._arena.data_ptr(), self._offsets
        x0 = torch.empty(B, K + 1, self.embed_dim, device=dev, dtype=torch.float32)
        check(lib().mfvit_patch_keep_embed(pk, ptr(img), ptr(idx), a + 4 * off["cls_token"][0], a + 4 * off["pos_embed"][0],
                                           a + 4 * off["patch_embed.proj.weight"][0], a + 4 * off["patch_embed.proj.bias"][0], ptr(fws),
                                           int(bool(save)), ptr(x0), ptr(self._keep_err), stream()), "mfvit_patch_keep_embed")
        if not save:
            self._release_ws(fws)
            fws = None
        return x0, (K + 1, pk, fws, idx)

    def _forward_chain(self, img, idx, plan, forced, save, drop=None, want_dimg=False):
        """Every encoder forward: (features (B, T_last, D), state).  idx: the kept patches of an active patch dropout (the front end then makes
        the first range's x0) or None (the first range takes the image); plan: [(block_lo, block_hi, tokens)] as _token_segments gives it - one
        range [0, depth) without token pruning.  The ranges run through mfvit_vit_forward_seg, each on a workspace of its own; behind every range
        but the last the rows are scored by the cls attention of its last block (read in place from the range's workspace), selected and
        reorganised (csrc/token_prune.hip); forced: checked selections (_check_token_indices) or None.
        state (None without save), for the backward: (ranges, stages, front, fuse, pruning) - per range (mfvit_vit_seg, workspace), per stage
        (idx_keep, idx_drop, w, T, K) on the device, the front end's tuple of _keep_embed or None, and which pool policy the range workspaces
        are under."""
        img = self._prep_img(img)
        dev = img.device
        cfg = self._cfg(img, save)
        self._ensure_shadow(cfg)
        B, D, fuse = img.shape[0], self.embed_dim, int(self.token_fuse)
        pruning = self.token_pruning_active()
        if (idx is not None or pruning) and (self._keep_err is None or self._keep_err.device != dev):
            self._keep_err = torch.zeros(1, device=dev, dtype=torch.int32)
        segs = [_lib.VitSeg(lo, hi, T, int(i == 0 and idx is None)) for i, (lo, hi, T) in enumerate(plan)]
        sizes = [lib().mfvit_vit_workspace_bytes_seg(cfg, drop, seg, int(want_dimg and seg.image_in)) for seg in segs]
        if 0 in sizes:
            raise _lib.MfvitError("invalid encoder configuration (image size must be a multiple of 16, dim 384 or 768, head_dim 32 / 64 / 96)")
        if pruning:
            self._retain_prune_sizes((bool(save), bool(want_dimg), drop is not None, B, idx is not None), sizes)
        x, front = (img, None) if idx is None else self._keep_embed(cfg, img, idx, save)
        params = self._kernel_params()
        H, HD = self.num_heads, D // self.num_heads
        ranges, stages = [], []
        for i, (seg, nbytes) in enumerate(zip(segs, sizes)):
            T = seg.tokens
            ws = self._take_ws(nbytes, dev)
            out = torch.empty(B, T, D, device=dev, dtype=torch.float32)
            check(lib().mfvit_vit_forward_seg(cfg, drop, seg, ptr(params), ptr(self._shadow), ptr(x), ptr(ws), ptr(out), stream()),
                  "mfvit_vit_forward_seg")
            x = out
            if i + 1 < len(segs):
                K = segs[i + 1].tokens - 1 - fuse
                lay = (ctypes.c_int64 * 4)()
                check(lib().mfvit_vit_attn_layout_seg(cfg, drop, seg, lay), "mfvit_vit_attn_layout_seg")
                last = (seg.block_hi - 1 - seg.block_lo) * lay[2]
                probs = torch.empty(B, T, device=dev, dtype=torch.float32)
                score = torch.empty(B, T - 1, device=dev, dtype=torch.float32)
                check(lib().mfvit_token_score(int(lay[3]), ws.data_ptr() + lay[0] + last, ws.data_ptr() + lay[1] + last, B, T, H, HD, ptr(probs),
                                              ptr(score), stream()), "mfvit_token_score")
                ik = torch.empty(B, K, device=dev, dtype=torch.int32)
                idr = torch.empty(B, T - 1 - K, device=dev, dtype=torch.int32)
                w = torch.empty(B, T - 1 - K, device=dev, dtype=torch.float32)
                check(lib().mfvit_token_select(ptr(score), T - 1, B, T - 1, K, ptr(forced[i]) if forced is not None else None, ptr(ik), ptr(idr),
                                               ptr(w), ptr(self._keep_err), stream()), "mfvit_token_select")
                x = torch.empty(B, 1 + K + fuse, D, device=dev, dtype=torch.float32)
                check(lib().mfvit_token_reorg_fwd(ptr(out), ptr(ik), ptr(idr), ptr(w), ptr(x), B, T, D, K, fuse, ptr(self._keep_err), stream()),
                      "mfvit_token_reorg_fwd")
                stages.append((ik, idr, w, T, K))
            if save:
                ranges.append((seg, ws))
            else:
                (self._release_prune_ws if pruning else self._release_ws)(ws)
        if pruning:
            self.last_token_indices = [st[0].long() for st in stages]
            self._last_token_plan = (plan[0][2], bool(fuse))
        return x, ((ranges, stages, front, fuse, pruning) if save else None)

    def _run_forward(self, img, save, drop=None, want_dimg=False):
        """The full grid as one range: (features, its workspace - None without save)."""
        feats, state = self._forward_chain(img, None, [(0, self.depth, self.num_tokens)], None, save, drop, want_dimg)
        return feats, (state[0][0][1] if save else None)

    def _keep_embed_bwd(self, front, dx0, gflat, dimg, cfg):
        """The front end's backward (stage -1 under patch dropout): d cls_token, d pe_b, d pe_w into the gradient arena `gflat` (None: none), dimg."""
        T, pk, fws, idx = front
        off = self._offsets
        g = (lambda name: gflat.data_ptr() + 4 * off[name][0]) if gflat is not None else (lambda name: None)
        stop = bool(cfg.stop_grad_conv1) or gflat is None
        check(lib().mfvit_patch_keep_embed_bwd(pk, ptr(idx), ptr(fws), ptr(dx0), g("cls_token"), None if stop else g("patch_embed.proj.weight"),
                                               None if stop else g("patch_embed.proj.bias"), ptr(dimg), ptr(self._keep_err), stream()),
              "mfvit_patch_keep_embed_bwd")

    def _take_grad_arena(self):
        """The zeroed flat gradient arena of one backward."""
        # The flat gradient arena is reused from step to step (stable addresses: the optimizers' device tables stay valid) unless a
        # parameter still holds a gradient - accumulation over several backward passes, or a second pass through this encoder
        # inside one autograd run (MoCo-v3 feeds both views through the base encoder) - in which case a fresh one is allocated.
        # ALIASING CONTRACT: gradient tensors handed out by one backward are views of this arena and are overwritten
        # by the next backward once every parameter's .grad is None again.  A caller that keeps gradients outside .grad across steps
        # (torch.autograd.grad results, detached copies of views kept after zero_grad(set_to_none=True)) must clone them, or switch
        # the reuse off: MFVIT_GRAD_ARENA_REUSE=0 / model.reuse_grad_arena = False (a fresh arena per backward, 87 MB per encoder).
        reuse = getattr(self, "reuse_grad_arena", os.environ.get("MFVIT_GRAD_ARENA_REUSE", "1") != "0")
        ga = getattr(self, "_grad_arena", None) if reuse else None
        # (`_grad_arena_lent` covers the second case before autograd has accumulated the first pass's views into p.grad; it is
        # cleared by the next forward.)
        if (ga is not None and not getattr(self, "_grad_arena_lent", False) and ga.shape == self._arena.shape
                and ga.device == self._arena.device and all(p.grad is None for p in self._arena_params)):
            gflat = ga.zero_()
        else:
            gflat = torch.zeros_like(self._arena)
            if not getattr(self, "_grad_arena_lent", False):
                self._grad_arena = gflat
        self._grad_arena_lent = True
        return gflat

    def _stage_groups(self, staged):
        """The (hi, lo) stage groups of one backward, descending: one group, or with a stage hook groups of `_grad_bucket_layers` blocks."""
        if not staged:
            return [(self.depth, -1)]
        # stages depth (final norm), depth-1 .. 0 (blocks), -1 (embedding) run in groups of `_grad_bucket_layers` blocks: after
        # each group its (contiguous) gradient slice can be exchanged while the next group computes.  Every library call joins
        # its weight-gradient side stream at the end, so fewer, larger groups keep more of that overlap than one call per block.
        gb = max(1, int(getattr(self, "_grad_bucket_layers", 4)))
        out, hi = [], self.depth
        while hi >= -1:
            lo = max(hi - gb, -1) if hi == self.depth else max(hi - gb + 1, -1)
            if lo == 0:
                lo = -1                                   # the embedding stage rides with the last block group
            out.append((hi, lo))
            hi = lo - 1
        return out

    @staticmethod
    def _backward_calls(ranges, groups, depth, front=False):
        """The mfvit_vit_backward_seg calls of one backward, host arithmetic only.  ranges: [(block_lo, block_hi)] ascending, contiguous from 0
        to depth; groups: the (hi, lo) model-stage groups of _stage_groups; front: the patch-dropout front end ran in front of range 0.
        -> per group the list of (range index, stage_hi, stage_lo, then): a group's stages are cut at the range boundaries; a range's entry
        stage block_hi (from its dx_out; the final norm for the last range) rides with its top block, block_lo - 1 (what feeds its first block:
        the embedding for range 0) with that block.  then: what follows the call that reaches block_lo - 1 - "reorg" (mfvit_token_reorg_bwd
        into the range below), "front" (the front end's backward) - or None."""
        out, i = [], len(ranges) - 1
        for hi, lo in groups:
            calls = []
            while i >= 0:
                a, b = ranges[i]
                top = min(hi, b - 1)               # the highest block of this range inside the group
                if top < a or top < lo:
                    break
                s_hi = b if (top == b - 1 and (b < depth or hi == depth)) else top
                s_lo = (lo if a == 0 else a - 1) if max(lo, a) == a else lo
                if s_lo != a - 1:
                    calls.append((i, s_hi, s_lo, None))
                    break                          # the rest of this range belongs to the next group
                calls.append((i, s_hi, s_lo, "reorg" if i > 0 else "front" if front else None))
                i -= 1
            out.append(calls)
        return out

    def _grad_views(self, gflat):
        self._last_grad_arena = gflat
        # per-parameter views of the flat gradient arena, arena order: ONE C++ call for the 150 views (a Python loop of slice + view cost 0.3 ms
        # of host time per encoder and step - at 16 pairs per step the host, not the GPU, sets the pace); fresh tensor objects every time, so
        # autograd's AccumulateGrad can keep them as .grad without copying
        params = [mod._parameters[attr] for _, mod, attr in self._param_holders()]
        views = torch._utils._unflatten_dense_tensors(gflat, params)
        return [v if p.requires_grad else None for v, p in zip(views, params)]

    def _backward_chain(self, cfg, state, dfeats, drop=None, dimg=None, want_params=True, on_stage_done=None):
        """Every encoder backward, on the state of _forward_chain: the block ranges from the last down (mfvit_vit_backward_seg, the calls of
        _backward_calls), mfvit_token_reorg_bwd between two of them, the front end's backward behind the first when it ran; the stage hook
        (on_stage_done, or the model's _grad_stage_hook) after every stage group.  Returns per-parameter gradient views (arena order) of a fresh
        flat gradient arena.  drop: the forward's mfvit_vit_drop (or None).  dimg: (B,3,H,W) f32, overwritten with d loss / d img (the first
        range's workspace must have been sized with want_dimg).  want_params=False (needs dimg): the data-gradient-only backward - no gradient
        arena, every returned gradient None."""
        ranges, stages, front, fuse = state[:4]
        dev = dfeats.device
        dfeats = dfeats.contiguous()
        if dfeats.dtype != torch.float32:
            dfeats = dfeats.float()
        B, D = cfg.batch, self.embed_dim
        if not want_params and dimg is None:
            raise _lib.MfvitError("a backward without parameter gradients needs the image gradient")
        gflat = self._take_grad_arena() if want_params else None
        hook = (on_stage_done or getattr(self, "_grad_stage_hook", None)) if want_params else None
        params = self._kernel_params()
        dx_in = [None if seg.image_in else torch.empty(B, seg.tokens, D, device=dev, dtype=torch.float32) for seg, _ in ranges]
        cur = dfeats                               # the gradient of the output of the range being walked
        groups = self._stage_groups(hook is not None)
        for (hi, lo), calls in zip(groups, self._backward_calls([(s.block_lo, s.block_hi) for s, _ in ranges], groups, self.depth, front is not None)):
            for i, s_hi, s_lo, then in calls:
                seg, ws = ranges[i]
                # (the call that runs the embedding stage also writes the image gradient)
                check(lib().mfvit_vit_backward_seg(cfg, drop, seg, ptr(params), ptr(self._shadow), ptr(ws), ptr(cur), ptr(gflat), ptr(dx_in[i]),
                                                   ptr(dimg) if (seg.image_in and s_lo == -1) else None, s_hi, s_lo, stream()),
                      "mfvit_vit_backward_seg")
                if then == "reorg":
                    ik, idr, w, T, K = stages[i - 1]
                    cur = torch.empty(B, T, D, device=dev, dtype=torch.float32)
                    check(lib().mfvit_token_reorg_bwd(ptr(dx_in[i]), ptr(ik), ptr(idr), ptr(w), ptr(cur), B, T, D, K, fuse, ptr(self._keep_err),
                                                      stream()), "mfvit_token_reorg_bwd")
                elif then == "front":
                    self._keep_embed_bwd(front, dx_in[0], gflat, dimg, cfg)
            if hook is not None:
                hook(self, hi, lo, gflat)
        if not want_params:
            return [None] * len(self._arena_params)
        return self._grad_views(gflat)

    def _run_backward(self, cfg, ws, dfeats, on_stage_done=None, drop=None, dimg=None, want_params=True):
        """The backward of _run_forward: the full grid as one range on the workspace `ws` (from _get_ws(.., want_dimg=True) when dimg is given)."""
        state = ([(_lib.VitSeg(0, self.depth, self.num_tokens, 1), ws)], [], None, 0, False)
        return self._backward_chain(cfg, state, dfeats, drop, dimg, want_params, on_stage_done)

    def _run_backward_lora(self, cfg, ws, dfeats, drop=None, dimg=None):
        """The selective backward of a model with adapters whose arena parameters are all frozen (mfvit_vit_backward_lora): returns the
        adapters' gradients in the order of LoraState.params(), views of one fresh flat tensor (so that .grad accumulation is
        autograd's).  The dW_eff scratch (one gradient-arena-sized tensor) is kept from step to step."""
        lo = self._lora
        dfeats = dfeats.contiguous()
        if dfeats.dtype != torch.float32:
            dfeats = dfeats.float()
        if lo.dw is None or lo.dw.shape != self._arena.shape or lo.dw.device != self._arena.device:
            lo.dw = torch.empty_like(self._arena)
        grads = lo.new_grads(self._arena.device)
        req = lo.request(grads=grads)
        check(lib().mfvit_vit_backward_lora(cfg, drop, ptr(self._kernel_params()), ptr(self._shadow), ptr(ws), ptr(dfeats), req, ptr(lo.dw),
                                            ptr(dimg), self.depth, -1 if dimg is not None else 0, stream()), "mfvit_vit_backward_lora")
        return grads

    def _lora_grads_from_arena(self, cfg, gflat):
        """Adapters beside trainable arena parameters: the full backward has filled the gradient arena `gflat`; one batched launch
        contracts its adapted dW slices to dA / dB (mfvit_vit_lora_grad).  Correct, and slower than the selective backward: every weight
        gradient of every block is formed."""
        lo = self._lora
        grads = lo.new_grads(self._arena.device)
        req = lo.request(grads=grads)
        check(lib().mfvit_vit_lora_grad(cfg, req, ptr(gflat), stream()), "mfvit_vit_lora_grad")
        return grads

    # ------------------------------------------------------------------ public API (reference call sites)
    def _features(self, x, caller, keep_indices=None, token_indices=None):
        # activations are saved when a parameter or the image needs a gradient (saliency / FGSM with a frozen backbone: the image only)
        need_x = torch.is_grad_enabled() and x.requires_grad
        lo = self.__dict__.get("_lora")
        lora_params = lo.params() if lo is not None else []
        need = need_x or (torch.is_grad_enabled() and (any(p.requires_grad for p in self._arena_params) or
                                                       any(p.requires_grad for p in lora_params)))
        key = (x._version, need, need_x, self._param_version(), torch.is_grad_enabled())
        c = self._feat_cache
        self._feat_cache = None
        drop = self._draw_drop()            # (a fresh seed per training-mode forward with dropout; None otherwise)
        pin = self.__dict__.get("_keep_pin") if (self.training and keep_indices is None) else None
        # patch dropout: a draw of this forward's own makes it stochastic; a pinned draw (one per step, shared by both calls) does not
        idx = self._resolve_keep(x, keep_indices)
        stochastic = drop is not None or (idx is not None and pin is None)
        prune = self.token_pruning_active()
        if token_indices is not None and not prune:
            raise _lib.MfvitError("token_indices given, but no token pruning is active (token_keep_rate = 1.0 or no prune block)")
        forced = None
        if prune:
            if lo is not None:
                raise _lib.MfvitError("LoRA adapters together with token pruning are not built: the block ranges run on the plain parameter "
                                      "arena (set token_keep_rate = 1.0, or detach the adapters)")
            _lib.require_cuda(x)
            if token_indices is not None:
                forced = self._check_token_indices(token_indices, int(x.shape[0]), self.num_tokens if idx is None else idx.shape[1] + 1)
                stochastic = True                   # (a forced selection is never served from, or left in, the single-use cache)
            key = key + (self.token_keep_rate, tuple(self.token_prune_blocks), self.token_fuse)
        if c is not None and c[0] is x and c[1] == key and c[2] != caller and not stochastic and (c[4] if len(c) > 4 else None) is idx:
            # the reference runs every backbone twice per step on the same tensor (features3D then __call__, FUS:128+131);
            # without dropout the second result is head(first[:, 0]): computed once.  Single use: a repeated call of
            # the SAME method always recomputes.  (Training mode with dropout / drop path: two forwards with their own masks, as the reference.)
            return c[3]
        c = None
        self._grad_arena_lent = False
        if idx is not None:
            self.last_keep_indices = idx
        feats = _EncoderFn.apply(self, x, idx, forced, need, drop, *self._arena_params, *lora_params)
        self._feat_cache = None if stochastic else (x, key, caller, feats, idx)
        return feats

    def features3D(self, x, keep_indices=None, token_indices=None):
        """(B,3,H,W) -> (B, T, 384) tokens after the final LayerNorm (FUS:128,133; crossvit.py:130-146).  Training mode with patch dropout
        (patch_drop.prob > 0, or explicit keep_indices (B, K): distinct patch indices per image): (B, 1 + K, 384), cls and the kept patches.
        With token pruning (token_keep_rate < 1; train() and eval() alike): (B, token_schedule()[-1], 384) - cls, the rows kept by every stage
        and, with token_fuse, the fused rows; last_token_indices / token_origin() say which.  token_indices: the selections to use instead of
        the model's own (the structure of last_token_indices), for tests and for reproducing a run."""
        return self._features(x, "features3D", keep_indices, token_indices)

    def forward_head(self, feats):
        h = self.head
        if isinstance(h, nn.Linear) and h.weight.dtype == torch.float32 and feats.is_cuda:
            # every plain Linear head (3 classes after MAIN_CA:309, the constructor's default 1000, BLD:29's mlp_dim before it is
            # replaced) runs on the row-dot head kernels over the cls rows: no rocBLAS call on the product path
            return _HeadFn.apply(feats, h.weight, h.bias)
        return h(feats[:, 0])      # a module the caller installed (MoCo's projector MLP: HIP Linear / BatchNorm nodes of its own)

    def forward(self, x, keep_indices=None, token_indices=None):
        """head(features3D(x)[:, 0])  (timm forward_features + head; training mode applies the dropout / drop-path / patch-dropout rates)."""
        return self.forward_head(self._features(x, "forward", keep_indices, token_indices))

    # ------------------------------------------------------------------ attention maps (include/mfvit.h, mfvit_vit_forward_attn)
    # All three run one evaluation forward (no dropout site, whatever self.training says) under no_grad, draw no seed, and leave the feature
    # cache and the module's state as they were.  Heads in timm's order; tokens: cls, then the patches row by row.
    def _attn_blocks(self, blocks):
        if blocks is None:
            return list(range(self.depth))
        out = set()
        for i in blocks:
            try:
                if isinstance(i, bool):
                    raise TypeError
                i = operator.index(i)
            except TypeError:
                raise ValueError(f"block indices must be integers, got {i!r}") from None
            if not -self.depth <= i < self.depth:
                raise ValueError(f"block index {i} out of range for depth {self.depth}")
            out.add(i % self.depth)
        if not out:
            raise ValueError("no block requested")
        return sorted(out)

    def _attn_forward(self, x, blocks, fuse, cls_only, rollout):
        self._refuse_if_pruning("an attention map / rollout")
        img = self._prep_img(x.detach())
        with torch.no_grad():
            cfg = self._cfg(img, False)
            cache = self._feat_cache
            self._ensure_shadow(cfg)
            self._feat_cache = cache            # (a rebuilt shadow means new parameters: the cache key no longer matches anyway)
            B, T, H = img.shape[0], self.num_tokens, self.num_heads
            rows = 1 if cls_only else T
            per = B * (1 if fuse else H) * rows * T
            dev = img.device
            maps = torch.empty(len(blocks) * per, device=dev, dtype=torch.float32) if blocks else None
            roll = torch.empty(B, T - 1, device=dev, dtype=torch.float32) if rollout else None
            req = _lib.VitAttnReq(sum(1 << l for l in blocks), fuse, int(cls_only), ptr(maps), ptr(roll), None)
            nbytes = lib().mfvit_vit_attn_scratch_bytes(cfg, req)
            if nbytes == 0:
                raise _lib.MfvitError("invalid attention-map request for this encoder configuration")
            scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            req.scratch = scratch.data_ptr()
            ws = self._get_ws(cfg)
            feats = torch.empty(B, T, self.embed_dim, device=dev, dtype=torch.float32)
            try:
                check(lib().mfvit_vit_forward_attn(cfg, req, ptr(self._kernel_params()), ptr(self._shadow), ptr(img), ptr(ws), ptr(feats), stream()),
                      "mfvit_vit_forward_attn")
            finally:
                self._release_ws(ws)
        shape = ((B,) if fuse else (B, H)) + ((T,) if cls_only else (T, T))
        return [maps[i * per:(i + 1) * per].view(shape) for i in range(len(blocks))], roll

    def get_attention_maps(self, x, blocks=None, head_fusion=None, cls_only=False):
        """Softmax probabilities of the blocks in `blocks` (indices, negative ones counted from the end; default: all), one f32 tensor per
        block in block order: (B, H, T, T), or (B, T, T) fused over the heads with head_fusion 'mean' | 'max' | 'min'; cls_only keeps the
        cls query's row only: (B, H, T) / (B, T).  The probabilities are recomputed on the GPU from each block's own attention forward."""
        if head_fusion not in _lib.HEAD_FUSION:
            raise ValueError(f"head_fusion must be None, 'mean', 'max' or 'min', got {head_fusion!r}")
        blocks = self._attn_blocks(blocks)
        return self._attn_forward(x, blocks, _lib.HEAD_FUSION[head_fusion], bool(cls_only), False)[0]

    def get_last_selfattention(self, x):
        """(B, H, T, T) attention probabilities of the last block (DINO's get_last_selfattention; [:, :, 0, 1:] are its cls maps)."""
        return self.get_attention_maps(x, blocks=[self.depth - 1])[0]

    def attention_rollout(self, x, head_fusion="mean"):
        """(B, gh, gw) cls row of the attention rollout over all blocks (Abnar & Zuidema 2020; include/mfvit.h): per block the heads fused
        by 'mean' | 'max' | 'min', half identity added, rows normalised, the blocks multiplied from the last down.  Not normalised: scale
        it for display (e.g. divide by its max)."""
        if head_fusion not in ("mean", "max", "min"):
            raise ValueError(f"head_fusion must be 'mean', 'max' or 'min', got {head_fusion!r}")
        _, roll = self._attn_forward(x, [], _lib.HEAD_FUSION[head_fusion], False, True)
        return roll.view(roll.shape[0], self.img_size[0] // 16, self.img_size[1] // 16)

    # ------------------------------------------------------------------ attention relevance (include/mfvit.h, mfvit_vit_backward_rel)
    # Chefer, Gur & Wolf 2021 (self-attention rule) for the score y_t = head(features3D(x)[:, 0])[t]: an evaluation forward with saved activations,
    # d y_t / d features through the head by autograd on a detached leaf copy of the features (the head in eval mode), then the data-gradient chain
    # with a relevance step behind every block's attention backward.  No dropout site, no seed, no p.grad, no gradient arena; the feature cache
    # and the module's state are left as they were.
    def _head_width(self):
        """Number of outputs of the head, when its modules tell (None otherwise)."""
        h = self.head
        for m in reversed(list(h.modules())):
            for a in ("out_features", "num_features"):
                v = getattr(m, a, None)
                if isinstance(v, int) and not isinstance(v, bool):
                    return v
        return None

    def _rel_forward(self, x):
        """Evaluation forward with saved activations: (cfg, workspace, features).  The caller releases the workspace."""
        self._refuse_if_pruning("a relevance map, hidden state or attention statistic")
        img = self._prep_img(x.detach())
        with torch.no_grad():
            cfg = self._cfg(img, True)
            cache = self._feat_cache
            self._ensure_shadow(cfg)
            self._feat_cache = cache            # (a rebuilt shadow means new parameters: the cache key no longer matches anyway)
            ws = self._get_ws(cfg)
            feats = torch.empty(img.shape[0], self.num_tokens, self.embed_dim, device=img.device, dtype=torch.float32)
            try:
                check(lib().mfvit_vit_forward(cfg, ptr(self._kernel_params()), ptr(self._shadow), ptr(img), ptr(ws), ptr(feats), stream()),
                      "mfvit_vit_forward")
            except BaseException:
                self._release_ws(ws)
                raise
        return cfg, ws, feats

    def _rel_backward(self, cfg, ws, dfeats, blocks, want_rel):
        """mfvit_vit_backward_rel on the workspace of _rel_forward: ([(B, T, T) map of every block in `blocks`], (B, T-1) relevance or None)."""
        B, T = cfg.batch, self.num_tokens
        dev = ws.device
        dfeats = dfeats.detach().float().contiguous()
        per = B * T * T
        with torch.no_grad():
            maps = torch.empty(len(blocks) * per, device=dev, dtype=torch.float32) if blocks else None
            rel = torch.empty(B, T - 1, device=dev, dtype=torch.float32) if want_rel else None
            req = _lib.VitRelReq(sum(1 << l for l in blocks), ptr(maps), ptr(rel), None)
            nbytes = lib().mfvit_vit_rel_scratch_bytes(cfg, req)
            if nbytes == 0:
                raise _lib.MfvitError("invalid relevance request for this encoder configuration")
            scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            req.scratch = scratch.data_ptr()
            check(lib().mfvit_vit_backward_rel(cfg, req, ptr(self._kernel_params()), ptr(self._shadow), ptr(ws), ptr(dfeats), stream()),
                  "mfvit_vit_backward_rel")
        return [maps[i * per:(i + 1) * per].view(B, T, T) for i in range(len(blocks))], rel

    def _relevance(self, x, target, blocks, want_rel):
        tgt = check_target(target, int(x.shape[0]) if x.dim() else 0, self._head_width())
        cfg, ws, feats = self._rel_forward(x)
        try:
            f = feats.detach().requires_grad_(True)
            with torch.enable_grad(), eval_modules(self.head):
                out = self.forward_head(f)
                idx = resolve_target(tgt, out)
                (df,) = torch.autograd.grad(out.gather(1, idx).sum(), f)
            return self._rel_backward(cfg, ws, df, blocks, want_rel)
        finally:
            self._release_ws(ws)

    def attention_relevance(self, x, target=None):
        """(B, gh, gw) class-specific relevance of the patches (Chefer et al. 2021, include/mfvit.h): the cls row of
        R = (I + A_{L-1}) ... (I + A_0), A_l = mean over heads of max(0, P o d y_t / d P), for the logit y_t of class `target` (None: the
        argmax of the head's output per image; an int; or a (B,) integer tensor).  Not normalised: scale it for display."""
        _, rel = self._relevance(x, target, [], True)
        return rel.view(rel.shape[0], self.img_size[0] // 16, self.img_size[1] // 16)

    def get_relevance_maps(self, x, target=None, blocks=None):
        """A_l = mean over heads of max(0, P o d y_t / d P) of the blocks in `blocks` (indices as in get_attention_maps; default: all), one
        (B, T, T) f32 tensor per block in block order; target as in attention_relevance."""
        blocks = self._attn_blocks(blocks)
        return self._relevance(x, target, blocks, False)[0]

    # ------------------------------------------------------------------ hidden states (include/mfvit.h, mfvit_vit_hidden_layout)
    # The f32 residual stream of every layer, as an evaluation forward with saved activations leaves it in its workspace (the pattern of
    # _rel_forward: no dropout site, no seed, no_grad, the feature cache and the module's state left as they were).
    def _hidden_view(self, cfg, ws):
        """(depth + 1, B, T, D) f32 view INTO the workspace of a saved-activations forward: valid until the workspace is released."""
        out = (ctypes.c_int64 * 2)()
        check(lib().mfvit_vit_hidden_layout(cfg, out), "mfvit_vit_hidden_layout")
        B, T, D = cfg.batch, self.num_tokens, self.embed_dim
        f = ws[out[0]:out[0] + self.depth * out[1] + B * T * D * 4].view(torch.float32)
        return f.as_strided((self.depth + 1, B, T, D), (out[1] // 4, T * D, D, 1))

    def hidden_states(self, x):
        """(B,3,H,W) -> (depth + 1, B, T, D) f32: hidden state 0 is cls + patch embedding + pos_embed (the input of block 0), hidden state l
        the output of block l - 1, before the final norm.  f32 in every precision.  A copy: the workspace goes back to the pool."""
        cfg, ws, _ = self._rel_forward(x)
        try:
            return self._hidden_view(cfg, ws).clone()
        finally:
            self._release_ws(ws)

    # ------------------------------------------------------------------ per-head attention statistics (include/mfvit.h, mfvit_attention_stats)
    # The pattern of hidden_states: an evaluation forward with saved activations, then one statistics launch that reads every block's qkv and
    # log-sum-exp in place from the workspace (mfvit_vit_attn_layout).  The per-head maps are never formed.
    def _attention_stats(self, cfg, ws, blocks):
        """(len(blocks), B, H, 6) float64 statistics of the (sorted) blocks from the workspace of a saved-activations forward."""
        from . import attnstats
        out = (ctypes.c_int64 * 4)()
        check(lib().mfvit_vit_attn_layout(cfg, out), "mfvit_vit_attn_layout")
        # one launch over the evenly spaced blocks lo, lo + step, .. that hold every requested one
        lo, step = blocks[0], 1
        if len(blocks) > 1:
            step = math.gcd(*(b - lo for b in blocks[1:]))
        span = list(range(lo, blocks[-1] + 1, step))
        gh, gw = self.img_size[0] // 16, self.img_size[1] // 16
        st = attnstats.attention_stats(ws[out[0] + lo * out[2]:], ws[out[1] + lo * out[2]:].view(torch.float32), int(out[3]), cfg.batch,
                                       self.num_tokens, self.num_heads, self.embed_dim // self.num_heads, (gh, gw), 16.0, len(span),
                                       (step * out[2], step * out[2]))
        if len(span) != len(blocks):
            st = st[torch.tensor([span.index(b) for b in blocks], device=st.device)]
        return st

    def attention_stats(self, x, blocks=None):
        """(B,3,H,W) -> {name: (len(blocks), B, heads) float64 cuda tensor} for the names of mfvit.attnstats.STATS: mean attention distance in
        pixels (cls row and column dropped; 'distance' as the public ViT notebook computes it, 'distance_renorm' with every row renormalised
        over the patches), mean row entropy and the cls row's entropy in nats, the mass the patches send to cls, and the mean diagonal mass -
        per image and head, of the blocks in `blocks` (indices as in get_attention_maps; default: all) in block order.  One evaluation
        forward (no dropout site, whatever self.training says) under no_grad; the feature cache and the module's state stay as they were."""
        from . import attnstats
        blocks = self._attn_blocks(blocks)
        cfg, ws, _ = self._rel_forward(x)
        try:
            with torch.no_grad():
                st = self._attention_stats(cfg, ws, blocks)
        finally:
            self._release_ws(ws)
        return {name: st[..., i].contiguous() for i, name in enumerate(attnstats.STATS)}

    def _final_norm(self, h):
        """The encoder's final LayerNorm of f32 rows (.., D), through mfvit_layernorm_fwd."""
        rows = h.reshape(-1, self.embed_dim).contiguous()
        with torch.no_grad():
            y, _, _ = ops.layernorm_fwd(rows, self.norm.weight.detach(), self.norm.bias.detach(), 1e-6)
        return y.view(h.shape)

    def get_intermediate_layers(self, x, n=1, reshape=False, return_prefix_tokens=False, norm=False):
        """timm's get_intermediate_layers: a tuple of the (B, T-1, D) patch tokens at the output of the last `n` blocks (int) or of the
        blocks in `n` (a sequence of indices, negative ones counted from the end), in block order.  reshape: (B, D, gh, gw) each;
        return_prefix_tokens: (patches, cls) pairs with cls (B, 1, D); norm: the encoder's final LayerNorm applied to every output."""
        if isinstance(n, bool):
            raise ValueError(f"n must be an int or a sequence of block indices, got {n!r}")
        if isinstance(n, int):
            if not 1 <= n <= self.depth:
                raise ValueError(f"n = {n} out of range for depth {self.depth}")
            blocks = list(range(self.depth - n, self.depth))
        else:
            blocks = self._attn_blocks(n)
        hs = self.hidden_states(x)
        outs = [hs[l + 1] for l in blocks]
        if norm:
            outs = [self._final_norm(o) for o in outs]
        prefix = [o[:, :1] for o in outs]
        outs = [o[:, 1:] for o in outs]
        if reshape:
            gh, gw = self.img_size[0] // 16, self.img_size[1] // 16
            outs = [o.reshape(o.shape[0], gh, gw, -1).permute(0, 3, 1, 2).contiguous() for o in outs]
        return tuple(zip(outs, prefix)) if return_prefix_tokens else tuple(outs)
