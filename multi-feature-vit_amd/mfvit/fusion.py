"""Two-stream fusion engine: one autograd node over mfvit_fusion_ex_forward / mfvit_fusion_ex_backward (f32).

The node's parameters are the LIVE tail of the Fus_CrossViT arena: the last multi-scale encoder's cross_attn_depth layers and the two
heads (FUS:137-139: only the last encoder's output is used).  The earlier encoders never enter the graph, so their .grad stays None."""
import torch

from . import _lib
from ._lib import FusionCfg, check, lib, ptr, stream

DIMS = (384, 768)
HEADS = (3, 6, 12)
MAX_CROSS_ATTN_DEPTH = 16   # csrc/fusion.hip MAX_XDEPTH


def fusion_cfg(B, T, C, dim=384, heads=3):
    c = FusionCfg()
    c.batch, c.tokens, c.dim, c.heads, c.num_classes = B, T, dim, heads, C
    c.eps_pre, c.eps_post = 1e-5, 1e-6
    return c


def check_fusion_shape(dim, heads):
    """The widths / head counts the exchange kernels are instantiated for."""
    if dim not in DIMS:
        raise NotImplementedError(f"the fused exchange is built for dim in {DIMS} (vit_small / vit_base), got {dim}")
    if heads not in HEADS:
        raise NotImplementedError(f"the fused exchange is built for heads in {HEADS}, got {heads}")


class FusionSpec:
    """What one FusionFn call needs besides tensors: the arena, where its live tail starts, and the exchange shape."""

    def __init__(self, arena, first_live, dim, heads, depth, pool_mean):
        self.arena, self.first_live = arena, first_live
        self.dim, self.heads, self.depth, self.pool_mean = dim, heads, depth, int(pool_mean)

    def live(self):
        return self.arena.params[self.first_live:]

    def tail(self, flat):
        off = self.arena.offsets[self.arena.named[self.first_live][0]][0]
        return flat[off:], off

    def grad_views(self, gtail, off):
        out = []
        for name, p in self.arena.named[self.first_live:]:
            if p.requires_grad:
                o, n = self.arena.offsets[name]
                out.append(gtail[o - off:o - off + n].view(p.shape))
            else:
                out.append(None)
        return out


class FusionFn(torch.autograd.Function):
    """(f_cxr, f_enh, backbone heads, live fusion params) -> (fused, x_cxr, x_enh)   [FUS:126-157]"""

    @staticmethod
    def forward(ctx, spec, f_cxr, f_enh, hw_c, hb_c, hw_e, hb_e, *params):
        _lib.require_cuda(f_cxr, f_enh)
        B, T, D = f_cxr.shape
        if D != spec.dim:
            raise _lib.MfvitError(f"fusion built for dim {spec.dim}, features have {D}")
        flat, off = spec.tail(spec.arena.ensure())
        L = spec.depth
        C = (flat.numel() - L * (8 * D * D + 10 * D)) // (2 * (D + 1))
        cfg = fusion_cfg(B, T, C, D, spec.heads)
        if lib().mfvit_fusion_ex_param_count(cfg, L, spec.pool_mean) != flat.numel():
            raise _lib.MfvitError("fusion parameter arena does not match the C ABI layout")
        f_cxr = f_cxr.contiguous().float()
        f_enh = f_enh.contiguous().float()
        ws = torch.empty(lib().mfvit_fusion_ex_workspace_bytes(cfg, L, spec.pool_mean), device=f_cxr.device, dtype=torch.uint8)
        fused = torch.empty(B, C, device=f_cxr.device, dtype=torch.float32)
        have_heads = hw_c is not None and hw_e is not None
        x_c = torch.empty_like(fused) if have_heads else None
        x_e = torch.empty_like(fused) if have_heads else None
        check(lib().mfvit_fusion_ex_forward(cfg, L, spec.pool_mean, ptr(flat), ptr(f_cxr), ptr(f_enh), ptr(hw_c), ptr(hb_c), ptr(hw_e),
                                            ptr(hb_e), ptr(ws), ptr(fused), ptr(x_c), ptr(x_e), stream()), "mfvit_fusion_ex_forward")
        ctx.spec, ctx.cfg, ctx.ws = spec, cfg, ws
        ctx.have_heads = have_heads
        ctx.save_for_backward(f_cxr, f_enh, hw_c, hw_e)
        if not have_heads:
            x_c = fused.new_zeros(B, C)
            x_e = fused.new_zeros(B, C)
        return fused, x_c, x_e

    @staticmethod
    def backward(ctx, dfused, dx_c, dx_e):
        f_cxr, f_enh, hw_c, hw_e = ctx.saved_tensors
        spec, cfg = ctx.spec, ctx.cfg
        flat, off = spec.tail(spec.arena.ensure())
        need_df = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        # ONE zeroed buffer for every accumulated gradient of this node (the live fusion parameters + the four head tensors): one fill launch
        # per step instead of five; every view starts 16-byte aligned
        sizes = [flat.numel()]
        want = [False] * 4
        if ctx.have_heads:
            want = [bool(ctx.needs_input_grad[i]) for i in (3, 4, 5, 6)]
            sizes += [hw_c.numel() if want[0] else 0, hw_c.shape[0] if want[1] else 0, hw_e.numel() if want[2] else 0, hw_e.shape[0] if want[3] else 0]
        offs, tot = [], 0
        for n in sizes:
            offs.append(tot)
            tot += (n + 3) // 4 * 4
        zbuf = torch.zeros(tot, device=flat.device, dtype=torch.float32)
        gflat = zbuf[:flat.numel()]
        df_c = torch.empty_like(f_cxr) if need_df else None
        df_e = torch.empty_like(f_enh) if need_df else None
        dhw_c = dhb_c = dhw_e = dhb_e = None
        if ctx.have_heads:
            if want[0]:
                dhw_c = zbuf[offs[1]:offs[1] + hw_c.numel()].view_as(hw_c)
            if want[1]:
                dhb_c = zbuf[offs[2]:offs[2] + hw_c.shape[0]]
            if want[2]:
                dhw_e = zbuf[offs[3]:offs[3] + hw_e.numel()].view_as(hw_e)
            if want[3]:
                dhb_e = zbuf[offs[4]:offs[4] + hw_e.shape[0]]
        dfused = dfused.contiguous().float()
        dx_c = dx_c.contiguous().float() if ctx.have_heads else None
        dx_e = dx_e.contiguous().float() if ctx.have_heads else None
        check(lib().mfvit_fusion_ex_backward(cfg, spec.depth, spec.pool_mean, ptr(flat), ptr(f_cxr), ptr(f_enh),
                                             ptr(hw_c) if ctx.have_heads else None, ptr(hw_e) if ctx.have_heads else None, ptr(ctx.ws),
                                             ptr(dfused), ptr(dx_c), ptr(dx_e), ptr(gflat), ptr(df_c), ptr(df_e), ptr(dhw_c), ptr(dhb_c),
                                             ptr(dhw_e), ptr(dhb_e), stream()), "mfvit_fusion_ex_backward")
        ctx.ws = None
        return (None, df_c, df_e, dhw_c, dhb_c, dhw_e, dhb_e) + tuple(spec.grad_views(gflat, off))


class ExchangeRun:
    """One mfvit_fusion_ex_forward called directly (no autograd node, so FusionFn runs what it always ran) whose workspace stays alive for the
    exchange-map calls of include/mfvit.h: attention() after the forward, grad_attention() after backward().  heads: the backbones' plain
    classifier heads (hw_c, hb_c, hw_e, hb_e) or None, as FusionFn takes them."""

    def __init__(self, spec, f_cxr, f_enh, heads=None):
        _lib.require_cuda(f_cxr, f_enh)
        B, T, D = f_cxr.shape
        if D != spec.dim:
            raise _lib.MfvitError(f"fusion built for dim {spec.dim}, features have {D}")
        self.spec = spec
        self.flat, _ = spec.tail(spec.arena.ensure())
        L = spec.depth
        C = (self.flat.numel() - L * (8 * D * D + 10 * D)) // (2 * (D + 1))
        self.cfg = cfg = fusion_cfg(B, T, C, D, spec.heads)
        if lib().mfvit_fusion_ex_param_count(cfg, L, spec.pool_mean) != self.flat.numel():
            raise _lib.MfvitError("fusion parameter arena does not match the C ABI layout")
        self.f_cxr, self.f_enh = f_cxr.detach().contiguous().float(), f_enh.detach().contiguous().float()
        dev = self.f_cxr.device
        self.ws = torch.empty(lib().mfvit_fusion_ex_workspace_bytes(cfg, L, spec.pool_mean), device=dev, dtype=torch.uint8)
        self.fused = torch.empty(B, C, device=dev, dtype=torch.float32)
        self.heads = heads
        self.x_c = torch.empty_like(self.fused) if heads is not None else None
        self.x_e = torch.empty_like(self.fused) if heads is not None else None
        hw_c, hb_c, hw_e, hb_e = heads if heads is not None else (None,) * 4
        check(lib().mfvit_fusion_ex_forward(cfg, L, spec.pool_mean, ptr(self.flat), ptr(self.f_cxr), ptr(self.f_enh), ptr(hw_c), ptr(hb_c),
                                            ptr(hw_e), ptr(hb_e), ptr(self.ws), ptr(self.fused), ptr(self.x_c), ptr(self.x_e), stream()),
              "mfvit_fusion_ex_forward")

    def attention(self, layer, fuse):
        """(2, B, heads, T), or (2, B, T) fused over the heads (fuse 1 mean | 2 max | 3 min): the softmax probabilities of exchange layer `layer`."""
        cfg = self.cfg
        shape = (2, cfg.batch, cfg.tokens) if fuse else (2, cfg.batch, cfg.heads, cfg.tokens)
        out = torch.empty(shape, device=self.ws.device, dtype=torch.float32)
        check(lib().mfvit_fusion_ex_attention(cfg, self.spec.depth, self.spec.pool_mean, ptr(self.ws), layer, fuse, ptr(out), stream()),
              "mfvit_fusion_ex_attention")
        return out

    def backward(self, dfused, dx_c=None, dx_e=None, need_df=False):
        """mfvit_fusion_ex_backward of (dfused, dx_c, dx_e) into a scratch parameter-gradient buffer that is dropped (the C ABI accumulates into
        one; no p.grad, no view of it leaves this call).  Returns (d / d f_cxr, d / d f_enh), or (None, None) without need_df."""
        spec, cfg = self.spec, self.cfg
        gflat = torch.zeros_like(self.flat)
        df_c = torch.empty_like(self.f_cxr) if need_df else None
        df_e = torch.empty_like(self.f_enh) if need_df else None
        have = self.heads is not None and dx_c is not None and dx_e is not None
        hw_c, _, hw_e, _ = self.heads if have else (None,) * 4
        dfused = dfused.contiguous().float()
        dx_c = dx_c.contiguous().float() if have else None
        dx_e = dx_e.contiguous().float() if have else None
        check(lib().mfvit_fusion_ex_backward(cfg, spec.depth, spec.pool_mean, ptr(self.flat), ptr(self.f_cxr), ptr(self.f_enh), ptr(hw_c),
                                             ptr(hw_e), ptr(self.ws), ptr(dfused), ptr(dx_c), ptr(dx_e), ptr(gflat), ptr(df_c), ptr(df_e),
                                             None, None, None, None, stream()), "mfvit_fusion_ex_backward")
        return df_c, df_e

    def grad_attention(self, layer):
        """(2, B, T): abar of exchange layer `layer` for the score the last backward() differentiated."""
        cfg = self.cfg
        abar = torch.empty(2, cfg.batch, cfg.tokens, device=self.ws.device, dtype=torch.float32)
        check(lib().mfvit_fusion_ex_grad_attention(cfg, self.spec.depth, self.spec.pool_mean, ptr(self.flat), ptr(self.f_cxr), ptr(self.f_enh),
                                                   ptr(self.ws), layer, ptr(abar), stream()), "mfvit_fusion_ex_grad_attention")
        return abar


def bimodal_relevance(maps_c, maps_e, abar):
    """mfvit_bimodal_relevance: maps_s (L_s, B, T, T) contiguous f32 relevance maps of each encoder, abar (2, B, T) -> (4, B, T-1) =
    rel_cc | rel_ce | rel_ec | rel_ee."""
    _lib.require_cuda(maps_c, maps_e, abar)
    Lc, B, T, _ = maps_c.shape
    Le = maps_e.shape[0]
    if tuple(maps_c.shape[1:]) != (B, T, T) or tuple(maps_e.shape[1:]) != (B, T, T) or tuple(abar.shape) != (2, B, T):
        raise _lib.MfvitError(f"bimodal relevance: maps {tuple(maps_c.shape)} / {tuple(maps_e.shape)} and abar {tuple(abar.shape)} do not agree")
    maps_c, maps_e, abar = maps_c.contiguous().float(), maps_e.contiguous().float(), abar.contiguous().float()
    nbytes = lib().mfvit_bimodal_relevance_scratch_bytes(B, T)
    if nbytes == 0:
        raise _lib.MfvitError(f"bimodal relevance is built for 2 .. 8192 tokens, got {T}")
    scratch = torch.empty(nbytes, device=abar.device, dtype=torch.uint8)
    out = torch.empty(4, B, T - 1, device=abar.device, dtype=torch.float32)
    check(lib().mfvit_bimodal_relevance(B, T, Lc, Le, ptr(maps_c), ptr(maps_e), ptr(abar), ptr(out), ptr(scratch), stream()),
          "mfvit_bimodal_relevance")
    return out
