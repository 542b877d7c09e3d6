"""Drop-in for the reference's two-stream fusion model file
(moco_pretraining/moco/model/crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_
changemodelinputlocation_std002_sum.py): ``MultiScaleTransformerEncoder`` and ``Fus_CrossViT`` with the same constructor
signatures, the same state-dict keys (22 at the defaults) and the same ``forward(vit_cxr, vit_enh, img_cxr, img_enh) -> (fused, x_cxr,
x_enh)`` contract, running on the gfx950 kernels of libmfvit_hip.so (csrc/fusion.hip + the ViT encoder).

Reference behaviours kept: the backbones are NOT submodules (Q1: only ``features3D`` bound
methods are stored, the modules arrive as forward arguments), so ``parameters()`` / ``state_dict()`` hold exactly the
fusion tensors; each backbone's two per-step evaluations on the same image are computed once (Q2); with one exchange layer and
pool='cls' only the cls row of the post-exchange LayerNorm / residual is consumed (Q3).

Constructor arguments as FUS:73-76: small_dim == large_dim in {384, 768} (vit_small / vit_base), heads in {3, 6, 12},
cross_attn_depth >= 1 (chained layers, FUS:40-63), multi_scale_enc_depth >= 1 (every encoder reads the backbone features and only the
last one's output is used, FUS:137-139: the earlier encoders are kept in the state dict but never run, so their .grad stays None),
pool in {'cls', 'mean'} (FUS:144-145).
"""
import os

import torch
import torch.nn as nn

from mfvit import _lib
from mfvit.arena import ParamArena
from mfvit.encoder import check_target, eval_modules, resolve_target
from mfvit.fusion import MAX_CROSS_ATTN_DEPTH, ExchangeRun, FusionFn, FusionSpec, bimodal_relevance, check_fusion_shape
from model.module import Attention, CrossAttention, FeedForward, PreNorm  # noqa: F401  (same import list as FUS:6)


class MultiScaleTransformerEncoder(nn.Module):
    """FUS:12-65.  ModuleList per layer: [0] PreNorm(CrossAttention) "cross_attn_s", [1] LayerNorm(eps 1e-6) "n_l",
    [2] PreNorm(CrossAttention) "cross_attn_l", [3] LayerNorm(eps 1e-6) "n_s"."""

    def __init__(self, small_dim=384, large_dim=384, cross_attn_depth=1, cross_attn_heads=3, dropout=0.):
        super().__init__()
        if small_dim != large_dim:
            # FUS:51,59 concatenate rows of both streams: the reference fails at forward; here at construction
            raise ValueError(f"small_dim ({small_dim}) must equal large_dim ({large_dim}): the exchange concatenates rows of both streams")
        check_fusion_shape(small_dim, cross_attn_heads)
        if not 1 <= cross_attn_depth <= MAX_CROSS_ATTN_DEPTH:
            raise NotImplementedError(f"cross_attn_depth must be in 1 .. {MAX_CROSS_ATTN_DEPTH}, got {cross_attn_depth}")
        self.dim, self.heads, self.depth = small_dim, cross_attn_heads, cross_attn_depth
        self.cross_attn_layers = nn.ModuleList([])
        for _ in range(cross_attn_depth):
            self.cross_attn_layers.append(nn.ModuleList([
                PreNorm(large_dim, CrossAttention(large_dim, num_heads=cross_attn_heads, attn_drop=dropout)),
                nn.LayerNorm(large_dim, eps=1e-6),
                PreNorm(small_dim, CrossAttention(small_dim, num_heads=cross_attn_heads, attn_drop=dropout)),
                nn.LayerNorm(small_dim, eps=1e-6),
            ]))

    def forward(self, xs, xl):
        from mfvit.xattn import exchange
        return exchange(self, xs, xl)


def _stochastic(vit):
    """True while a backbone draws dropout / drop-path masks (training mode with a rate > 0): every call is then a forward of its own."""
    f = getattr(vit, "is_stochastic", None)
    return bool(f()) if callable(f) else False


class Fus_CrossViT(nn.Module):
    def __init__(self, model_vit_cxr, model_vit_enh, num_classes=3, small_dim=384, large_dim=384, cross_attn_depth=1,
                 multi_scale_enc_depth=1, heads=3, dropout=0., pool='cls', patch_drop_shared=True):
        super().__init__()
        if pool not in ('cls', 'mean'):
            raise ValueError(f"pool must be 'cls' or 'mean', got {pool!r}")
        if multi_scale_enc_depth < 1:
            raise ValueError(f"multi_scale_enc_depth must be >= 1, got {multi_scale_enc_depth}")
        # bound methods, as in FUS:80,83: the backbones do not become submodules
        self.vit_features_cxr = model_vit_cxr.features3D
        self.vit_features_enh = model_vit_enh.features3D
        self.multi_scale_transformers = nn.ModuleList([
            MultiScaleTransformerEncoder(small_dim=small_dim, large_dim=large_dim, cross_attn_depth=cross_attn_depth,
                                         cross_attn_heads=heads, dropout=dropout)
            for _ in range(multi_scale_enc_depth)])
        self.pool = pool
        # patch dropout of the encoders (timm PatchDropout): one draw per encoder per step; True - both streams keep the SAME patches (the CXR and
        # its enhanced twin are pixel-aligned: the choice Mixup makes for partner and boxes), False - one set of indices per stream
        self.patch_drop_shared = bool(patch_drop_shared)
        self.num_classes = num_classes
        self.mlp_head_cxr = nn.Sequential(nn.Linear(small_dim, num_classes))
        self.mlp_head_enh = nn.Sequential(nn.Linear(large_dim, num_classes))
        self.apply(self._init_weights)
        self._arena = ParamArena(list(self.named_parameters()))
        # the live tail of the arena: the last encoder's layers + the two heads (named_parameters order)
        first_live = next(i for i, (n, _) in enumerate(self._arena.named)
                          if n.startswith(f"multi_scale_transformers.{multi_scale_enc_depth - 1}."))
        self._spec = FusionSpec(self._arena, first_live, small_dim, heads, cross_attn_depth, pool == 'mean')
        self._two_streams = os.environ.get("MFVIT_TWO_STREAMS", "1") == "1"
        self._side = None

    @staticmethod
    def _init_weights(m):  # FUS:117-124
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if getattr(self, "_arena", None) is not None:
            self._arena.rebuild()
        return out

    def flat_parameters(self):
        return self._arena.ensure()

    @staticmethod
    def _plain_head(vit):
        h = getattr(vit, "head", None)
        if isinstance(h, nn.Linear) and h.weight.dtype == torch.float32 and h.bias is not None:
            return h
        return None

    def _draw_patch_keep(self, vit_cxr, vit_enh, img_cxr, img_enh):
        """The kept-patch indices of this step for (vit_cxr, vit_enh), None where an encoder runs no patch dropout (eval(), rate 0, not one of
        ours).  Drawn once per step on the caller's stream: features3D and the head forward of a step share them."""
        def draw(vit, img):
            f = getattr(vit, "draw_keep_indices", None)
            return f(img.shape[0], img.device) if callable(f) and img is not None else None
        idx_c = draw(vit_cxr, img_cxr)
        if idx_c is not None and self.patch_drop_shared and callable(getattr(vit_enh, "draw_keep_indices", None)) and vit_enh.training \
                and vit_enh.patch_drop.prob > 0.0:
            if vit_enh.num_tokens != vit_cxr.num_tokens or vit_enh.patch_drop.num_keep(vit_enh.num_tokens - 1) != idx_c.shape[1] \
                    or img_enh is None or img_enh.shape[0] != idx_c.shape[0]:
                from mfvit._lib import MfvitError
                raise MfvitError("patch_drop_shared=True needs two encoders with the same patch grid and patch_drop_rate (and one batch size): "
                                 "build the model with patch_drop_shared=False for one draw per stream")
            return idx_c, idx_c
        return idx_c, draw(vit_enh, img_enh)

    @staticmethod
    def _check_token_pruning(vit_cxr, vit_enh):
        """Token pruning between blocks (VisionTransformerMoCo.token_keep_rate < 1): the exchange takes ONE token count (mfvit_fusion_cfg), so both
        encoders must prune alike - same grid, rate, blocks and fuse flag; each stream still selects by its own attention."""
        def plan(vit):
            f = getattr(vit, "token_pruning_active", None)
            if not callable(f) or not f():
                return None
            return {"token grid": vit.num_tokens, "token_keep_rate": float(vit.token_keep_rate),
                    "token_prune_blocks": tuple(vit.token_prune_blocks), "token_fuse": bool(vit.token_fuse)}
        pc, pe = plan(vit_cxr), plan(vit_enh)
        if pc == pe:
            return
        from mfvit._lib import MfvitError
        if pc is None or pe is None:
            raise MfvitError("token pruning is active in one encoder only: the exchange needs the same token count from both streams (set the "
                             "same token_keep_rate, token_prune_blocks and token_fuse on both)")
        diff = ", ".join(f"{k} {pc[k]!r} vs {pe[k]!r}" for k in pc if pc[k] != pe[k])
        raise MfvitError(f"the two encoders prune tokens differently ({diff}): the exchange needs the same token count from both streams")

    def forward(self, vit_cxr, vit_enh, img_cxr, img_enh):
        self._check_token_pruning(vit_cxr, vit_enh)
        idx_c, idx_e = self._draw_patch_keep(vit_cxr, vit_enh, img_cxr, img_enh)
        if idx_c is None and idx_e is None:
            return self._forward(vit_cxr, vit_enh, img_cxr, img_enh)
        import contextlib
        with contextlib.ExitStack() as pins:
            for vit, idx in ((vit_cxr, idx_c), (vit_enh, idx_e)):
                if idx is not None:
                    pins.enter_context(vit.pinned_keep_indices(idx))
            return self._forward(vit_cxr, vit_enh, img_cxr, img_enh)

    def _forward(self, vit_cxr, vit_enh, img_cxr, img_enh):
        two = bool(self._two_streams and img_enh is not None and img_enh.is_cuda)
        # grid-size hint for small batches - two encoders side by side - travels in the encoders' own call configuration (mfvit_vit_cfg.stream_share), not in a
        # process-wide setting: two models in one process do not fight over it
        for enc in (getattr(self.vit_features_cxr, "__self__", None), getattr(self.vit_features_enh, "__self__", None)):
            if enc is not None:
                enc._stream_share = 2 if two else 1
        if two:
            # the two encoders are independent: run the ENH stream's ~100 kernels on a second HIP stream so that its
            # MFMA phases overlap the CXR stream's HBM-bound epilogues (and vice versa); autograd replays each
            # encoder's backward on the stream its forward ran on, so the overlap holds for the backward too
            main = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream()
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                enh_ftrs = self.vit_features_enh(img_enh)  #             FUS:133
            cxr_ftrs = self.vit_features_cxr(img_cxr)      # (B, 197, dim) FUS:128
            main.wait_stream(self._side)
            enh_ftrs.record_stream(main)
        else:
            cxr_ftrs = self.vit_features_cxr(img_cxr)      # (B, 197, dim)   FUS:128
            enh_ftrs = self.vit_features_enh(img_enh)      #                 FUS:133
        hc, he = self._plain_head(vit_cxr), self._plain_head(vit_enh)
        fused_heads = hc is not None and he is not None and hc.out_features == self.num_classes == he.out_features \
            and getattr(vit_cxr, "features3D", None) == self.vit_features_cxr \
            and getattr(vit_enh, "features3D", None) == self.vit_features_enh \
            and not _stochastic(vit_cxr) and not _stochastic(vit_enh)
        # (a backbone in training mode with dropout / drop path: vit_S(img_S) is a forward of its own, with its own masks - FUS:131,135 call it
        # after features3D, as the reference does; the CA step then runs each backbone twice)
        if fused_heads:
            # x_S = vit_S(img_S) = head_S(features3D(img_S)[:, 0])  (FUS:131,135; dropouts are 0): evaluated inside the fused node
            return FusionFn.apply(self._spec, cxr_ftrs, enh_ftrs, hc.weight, hc.bias, he.weight, he.bias, *self._spec.live())
        fused, _, _ = FusionFn.apply(self._spec, cxr_ftrs, enh_ftrs, None, None, None, None, *self._spec.live())
        return fused, vit_cxr(img_cxr), vit_enh(img_enh)

    def attention_relevance(self, vit_cxr, vit_enh, img_cxr, img_enh, target=None):
        """(rel_cxr, rel_enh): the class-specific relevance (Chefer et al. 2021; VisionTransformerMoCo.attention_relevance) of each encoder's
        patches, (B, gh, gw) each, for the score the reference predicts from, y_t = (fused + x_cxr + x_enh)[t] (MAIN_CA:868-870); target: None
        (the argmax per image), an int or a (B,) integer tensor.  Each encoder runs an evaluation forward with saved activations; the fusion and
        the single-stream heads (in eval mode) run on leaf copies of the two feature tensors, and d y_t / d features of each stream feeds that
        encoder's relevance backward.  The exchange's own cross-attention is not part of the chain (cross_relevance is the form that has it).  No p.grad is set.  The two encoders run one
        after the other on the caller's stream, whatever _two_streams says.  vit_cxr / vit_enh must be the encoders this model was built with
        (forward takes the features from those): ValueError otherwise."""
        for vit, bound, name in ((vit_cxr, self.vit_features_cxr, "vit_cxr"), (vit_enh, self.vit_features_enh, "vit_enh")):
            if getattr(vit, "features3D", None) != bound:
                raise ValueError(f"{name} is not the encoder this Fus_CrossViT was built with: its relevance would not be the predicting model's")
        B = int(img_cxr.shape[0])
        if img_enh is None or int(img_enh.shape[0]) != B:
            raise ValueError("img_cxr and img_enh must hold the same number of images")
        tgt = check_target(target, B, self.num_classes)
        cfg_c, ws_c, f_c = vit_cxr._rel_forward(img_cxr)
        try:
            cfg_e, ws_e, f_e = vit_enh._rel_forward(img_enh)
            try:
                lc, le = f_c.detach().requires_grad_(True), f_e.detach().requires_grad_(True)
                with torch.enable_grad(), eval_modules(vit_cxr.head, vit_enh.head):
                    hc, he = self._plain_head(vit_cxr), self._plain_head(vit_enh)
                    if hc is not None and he is not None and hc.out_features == self.num_classes == he.out_features:
                        fused, x_c, x_e = FusionFn.apply(self._spec, lc, le, hc.weight, hc.bias, he.weight, he.bias, *self._spec.live())
                    else:
                        fused, _, _ = FusionFn.apply(self._spec, lc, le, None, None, None, None, *self._spec.live())
                        x_c, x_e = vit_cxr.forward_head(lc), vit_enh.forward_head(le)
                    out = fused + x_c + x_e
                    idx = resolve_target(tgt, out)
                    g_c, g_e = torch.autograd.grad(out.gather(1, idx).sum(), (lc, le))
                _, r_c = vit_cxr._rel_backward(cfg_c, ws_c, g_c, [], True)
                _, r_e = vit_enh._rel_backward(cfg_e, ws_e, g_e, [], True)
            finally:
                vit_enh._release_ws(ws_e)
        finally:
            vit_cxr._release_ws(ws_c)
        return (r_c.view(B, vit_cxr.img_size[0] // 16, vit_cxr.img_size[1] // 16),
                r_e.view(B, vit_enh.img_size[0] // 16, vit_enh.img_size[1] // 16))

    # ------------------------------------------------------------------ the exchange's own maps (include/mfvit.h, mfvit_fusion_ex_attention ..)
    # Key row 0 of an exchange map is the query's own cls token, rows 1 .. T-1 the OTHER stream's patch tokens, row by row; "cxr" is the direction
    # whose query is the CXR cls token.  All three calls run evaluation forwards of the encoders (no dropout site, no seed), call the fusion
    # library directly on a workspace of their own (forward() and its autograd node run what they always ran), set no p.grad, allocate no
    # gradient arena and leave the training flags, the RNG states and the encoders' feature caches as they were.
    def _check_pair(self, vit_cxr, vit_enh, img_cxr, img_enh):
        for vit, bound, name in ((vit_cxr, self.vit_features_cxr, "vit_cxr"), (vit_enh, self.vit_features_enh, "vit_enh")):
            if getattr(vit, "features3D", None) != bound:
                raise ValueError(f"{name} is not the encoder this Fus_CrossViT was built with: its maps would not be the predicting model's")
        B = int(img_cxr.shape[0])
        if img_enh is None or int(img_enh.shape[0]) != B:
            raise ValueError("img_cxr and img_enh must hold the same number of images")
        return B

    def _check_one_layer_cls(self, what):
        if self._spec.depth != 1 or self._spec.pool_mean:
            raise NotImplementedError(f"{what} is defined for cross_attn_depth == 1 and pool == 'cls' (got depth {self._spec.depth}, "
                                      f"pool {self.pool!r}); get_exchange_attention works at any depth and pooling")

    @staticmethod
    def _eval_features(vit, img):
        """features3D of an evaluation forward without saved activations, the feature cache left alone."""
        vit._refuse_if_pruning("an exchange map / cross-stream relevance")
        img = vit._prep_img(img.detach())
        with torch.no_grad():
            cfg = vit._cfg(img, False)
            cache = vit._feat_cache
            vit._ensure_shadow(cfg)
            vit._feat_cache = cache
            ws = vit._get_ws(cfg)
            feats = torch.empty(img.shape[0], vit.num_tokens, vit.embed_dim, device=img.device, dtype=torch.float32)
            try:
                _lib.check(_lib.lib().mfvit_vit_forward(cfg, _lib.ptr(vit._kernel_params()), _lib.ptr(vit._shadow), _lib.ptr(img), _lib.ptr(ws),
                                                        _lib.ptr(feats), _lib.stream()), "mfvit_vit_forward")
            finally:
                vit._release_ws(ws)
        return feats

    def _scored_exchange(self, vit_cxr, vit_enh, f_c, f_e, tgt, need_df):
        """The exchange forward on (f_c, f_e) and the backward of y_t = (fused + x_cxr + x_enh)[t]: (run, d y_t / d f_c, d y_t / d f_e)."""
        hc, he = self._plain_head(vit_cxr), self._plain_head(vit_enh)
        fused_heads = hc is not None and he is not None and hc.out_features == self.num_classes == he.out_features
        with torch.no_grad():
            run = ExchangeRun(self._spec, f_c, f_e, (hc.weight, hc.bias, he.weight, he.bias) if fused_heads else None)
        if fused_heads:
            with torch.no_grad():
                idx = resolve_target(tgt, run.fused + run.x_c + run.x_e)
                hot = torch.zeros_like(run.fused).scatter_(1, idx, 1.0)
                g_c, g_e = run.backward(hot, hot, hot, need_df)
            return run, g_c, g_e
        lc, le = run.f_cxr.detach().requires_grad_(True), run.f_enh.detach().requires_grad_(True)
        with torch.enable_grad(), eval_modules(vit_cxr.head, vit_enh.head):
            x = vit_cxr.forward_head(lc) + vit_enh.forward_head(le)
            idx = resolve_target(tgt, run.fused + x.detach())
            h_c, h_e = torch.autograd.grad(x.gather(1, idx).sum(), (lc, le)) if need_df else (None, None)
        with torch.no_grad():
            hot = torch.zeros_like(run.fused).scatter_(1, idx, 1.0)
            g_c, g_e = run.backward(hot, None, None, need_df)
            if need_df:
                g_c, g_e = g_c + h_c, g_e + h_e
        return run, g_c, g_e

    def get_exchange_attention(self, vit_cxr, vit_enh, img_cxr, img_enh, head_fusion=None):
        """[(a_cxr, a_enh) for every exchange layer of the live encoder]: the softmax probabilities of the cls queries exactly as the forward
        normalised them, (B, heads, T) each, or (B, T) fused over the heads with head_fusion 'mean' | 'max' | 'min' (max / min are not
        renormalised: a max-fused row sums to more than 1, a min-fused row to less).  Any cross_attn_depth, either pool."""
        self._check_pair(vit_cxr, vit_enh, img_cxr, img_enh)
        if head_fusion not in _lib.HEAD_FUSION:
            raise ValueError(f"head_fusion must be None, 'mean', 'max' or 'min', got {head_fusion!r}")
        fuse = _lib.HEAD_FUSION[head_fusion]
        with torch.no_grad():
            run = ExchangeRun(self._spec, self._eval_features(vit_cxr, img_cxr), self._eval_features(vit_enh, img_enh))
            try:
                out = [run.attention(l, fuse) for l in range(self._spec.depth)]
            finally:
                run.ws = None
        return [(a[0], a[1]) for a in out]

    def exchange_relevance(self, vit_cxr, vit_enh, img_cxr, img_enh, target=None):
        """(Abar_cxr, Abar_enh), (B, T) each: the gradient-weighted exchange map Abar[j] = mean over heads of max(0, a_h[j] d y_t / d a_h[j]) for
        the score of attention_relevance, y_t = (fused + x_cxr + x_enh)[t]; target as there.  cross_attn_depth == 1, pool == 'cls'."""
        B = self._check_pair(vit_cxr, vit_enh, img_cxr, img_enh)
        tgt = check_target(target, B, self.num_classes)
        self._check_one_layer_cls("exchange_relevance")
        run, _, _ = self._scored_exchange(vit_cxr, vit_enh, self._eval_features(vit_cxr, img_cxr), self._eval_features(vit_enh, img_enh), tgt, False)
        try:
            with torch.no_grad():
                abar = run.grad_attention(0)
        finally:
            run.ws = None
        return abar[0], abar[1]

    def cross_relevance(self, vit_cxr, vit_enh, img_cxr, img_enh, target=None):
        """(rel_cc, rel_ce, rel_ec, rel_ee), (B, gh, gw) each, not normalised: the relevance of each image's patches for y_t THROUGH the exchange
        (Chefer et al. 2021, self-attention rule inside the encoders, co-attention rule across the exchange; include/mfvit.h,
        mfvit_bimodal_relevance).  rel_cc / rel_ce: what the CXR cls token draws from the CXR / ENH patches, rel_ee / rel_ec likewise for the
        ENH cls token; the CXR image's total is rel_cc + rel_ec, the ENH image's rel_ee + rel_ce.  Keeps every block's (B, T, T) relevance
        map of both encoders while it runs: 4 (L_cxr + L_enh) B T^2 bytes.  cross_attn_depth == 1, pool == 'cls'."""
        B = self._check_pair(vit_cxr, vit_enh, img_cxr, img_enh)
        tgt = check_target(target, B, self.num_classes)
        self._check_one_layer_cls("cross_relevance")
        if vit_cxr.num_tokens != vit_enh.num_tokens:
            raise ValueError("the two encoders must produce the same number of tokens")
        cfg_c, ws_c, f_c = vit_cxr._rel_forward(img_cxr)
        try:
            cfg_e, ws_e, f_e = vit_enh._rel_forward(img_enh)
            try:
                run, g_c, g_e = self._scored_exchange(vit_cxr, vit_enh, f_c, f_e, tgt, True)
                try:
                    with torch.no_grad():
                        abar = run.grad_attention(0)
                finally:
                    run.ws = None
                m_c, _ = vit_cxr._rel_backward(cfg_c, ws_c, g_c, list(range(vit_cxr.depth)), False)
                m_e, _ = vit_enh._rel_backward(cfg_e, ws_e, g_e, list(range(vit_enh.depth)), False)
            finally:
                vit_enh._release_ws(ws_e)
        finally:
            vit_cxr._release_ws(ws_c)

        def stacked(ms):    # (the maps of one call are slices of one buffer, block after block)
            base = ms[0]._base
            return base.view(len(ms), *ms[0].shape) if base is not None and base.numel() == len(ms) * ms[0].numel() else torch.stack(ms)
        with torch.no_grad():
            out = bimodal_relevance(stacked(m_c), stacked(m_e), abar)
        gc, ge = (vit_cxr.img_size[0] // 16, vit_cxr.img_size[1] // 16), (vit_enh.img_size[0] // 16, vit_enh.img_size[1] // 16)
        return out[0].view(B, *gc), out[1].view(B, *ge), out[2].view(B, *gc), out[3].view(B, *ge)

    # ------------------------------------------------------------------ the perturbation test (mfvit.perturb; include/mfvit.h, mfvit_patch_rank ..)
    def perturbation_test(self, vit_cxr, vit_enh, img_cxr, img_enh, maps, target=None, fractions=None, mode="positive", fill=None,
                          max_batch=None, meter=None, return_logits=False, ks=None):
        """mfvit.perturb.perturbation_test for the two-stream model, scored on fused + x_cxr + x_enh (MAIN_CA:868), the score of
        attention_relevance: meter, or (meter, logits (S, B, classes)) with return_logits.  maps = (m_cxr, m_enh), each (B, gh, gw) or (B, P)
        for its own image; either may be None: that stream stays intact at every step - the stream-ablation curve.  Each stream has its own
        patch count (k_s = int(P * fractions[s]) per stream; the meter's fractions are those of the first perturbed stream) and its own fill:
        fill = None or (fill_cxr, fill_enh), each as perturb_patches takes it.  target, mode, max_batch (images per stream and forward),
        meter, ks as there.  Runs this model's ordinary forward under no_grad, everything in evaluation mode; training flags, RNG states, the
        encoders' feature caches and p.grad stay as they were."""
        from mfvit import perturb
        B = self._check_pair(vit_cxr, vit_enh, img_cxr, img_enh)
        if not isinstance(maps, (tuple, list)) or len(maps) != 2 or (maps[0] is None and maps[1] is None):
            raise ValueError("maps must be (m_cxr, m_enh), at least one of them a relevance map")
        if fill is not None and (not isinstance(fill, (tuple, list)) or len(fill) != 2):
            raise ValueError("fill must be None or (fill_cxr, fill_enh)")
        fills = (None, None) if fill is None else fill
        plans = [perturb._plan(img, m, fractions, ks, mode, max_batch, what)
                 for img, m, what in ((img_cxr, maps[0], "perturbation_test (cxr)"), (img_enh, maps[1], "perturbation_test (enh)"))]
        tgt = check_target(target, B, self.num_classes)
        lead = plans[0] if maps[0] is not None else plans[1]
        meter = perturb._meter_for(meter, lead[2], lead[1])
        _lib.require_cuda(img_cxr, img_enh, maps[0], maps[1])

        def forward(xs):
            fused, x_c, x_e = self(vit_cxr, vit_enh, xs[0], xs[1])
            return fused + x_c + x_e
        saved = [(v, v._feat_cache, getattr(v, "_grad_arena_lent", False)) for v in (vit_cxr, vit_enh)]
        try:
            with torch.no_grad(), eval_modules(self, vit_cxr, vit_enh):
                streams = [(img, None if m is None else perturb.patch_rank(m), perturb.ranges_for(P, counts, mode), f)
                           for img, m, (_, P, counts), f in zip((img_cxr, img_enh), maps, plans, fills)]
                logits = perturb.run_steps(forward, streams, len(lead[2]), B, max_batch, tgt, meter, mode == "insertion")
        finally:
            for v, cache, lent in saved:
                v._feat_cache, v._grad_arena_lent = cache, lent
        return (meter, logits) if return_logits else meter

    # ------------------------------------------------------------------ representation similarity (mfvit.similarity; include/mfvit.h, mfvit_gram_centered ..)
    def stream_similarity(self, vit_cxr, vit_enh, batches, tokens="all", unbiased=True):
        """Layer-wise minibatch linear CKA (Nguyen, Raghu & Kornblith 2021) of the two encoders' hidden states: {'cxr_enh': (Lc + 1, Le + 1),
        'cxr_cxr': (Lc + 1, Lc + 1), 'enh_enh': (Le + 1, Le + 1)} float64 arrays, entry [i, j] between hidden state i of the first and j of the
        second (VisionTransformerMoCo.hidden_states' numbering).  batches yields (img_cxr, img_enh) pairs of the same examples; tokens and
        unbiased as mfvit.similarity.cka.  One evaluation forward per encoder and minibatch, under no_grad; training flags, feature caches and
        p.grad stay as they were.  The exchange layers take no part: the similarity is between the backbones."""
        from mfvit import similarity

        def pairs():
            for b in batches:
                if torch.is_tensor(b) or len(b) != 2:
                    raise ValueError("stream_similarity takes (img_cxr, img_enh) pairs")
                yield b
        ce, cc, ee = similarity.layerwise([vit_cxr, vit_enh], pairs(), [(0, 1), (0, 0), (1, 1)], tokens, unbiased)
        return {"cxr_enh": ce, "cxr_cxr": cc, "enh_enh": ee}

    # ------------------------------------------------------------------ per-head attention statistics (mfvit.attnstats; include/mfvit.h, mfvit_attention_stats)
    def attention_stats(self, vit_cxr, vit_enh, batches):
        """Mean attention distance, entropy, cls mass and self mass of every head of every block of the two encoders (mfvit.attnstats.STATS;
        Dosovitskiy et al. 2021, Fig. 11): {'cxr': {name: (Lc, H) float64 array}, 'enh': {name: (Le, H)}}, per-image means over all batches.
        batches yields (img_cxr, img_enh) pairs.  One evaluation forward per encoder and batch, under no_grad, the statistics accumulated on
        the device; training flags, feature caches and p.grad stay as they were.  The exchange layers take no part."""
        from mfvit import attnstats
        vits = (vit_cxr, vit_enh)
        for vit, bound, name in ((vit_cxr, self.vit_features_cxr, "vit_cxr"), (vit_enh, self.vit_features_enh, "vit_enh")):
            if getattr(vit, "features3D", None) != bound:
                raise ValueError(f"{name} is not the encoder this Fus_CrossViT was built with: its heads would not be the predicting model's")
        meters = [attnstats.AttentionStatsMeter(v.depth, v.num_heads) for v in vits]
        for b in batches:
            if torch.is_tensor(b) or len(b) != 2:
                raise ValueError("attention_stats takes (img_cxr, img_enh) pairs")
            if int(b[0].shape[0]) != int(b[1].shape[0]):
                raise ValueError("img_cxr and img_enh must hold the same number of images")
            for vit, x, meter in zip(vits, b, meters):
                cfg, ws, _ = vit._rel_forward(x)
                try:
                    with torch.no_grad():
                        meter.update(vit._attention_stats(cfg, ws, list(range(vit.depth))))
                finally:
                    vit._release_ws(ws)
        if not meters[0].batches:
            raise ValueError("no batch")
        return {"cxr": meters[0].result(), "enh": meters[1].result()}

    # ------------------------------------------------------------------ gradient attribution (mfvit.attribution; include/mfvit.h, mfvit_attr_inputs ..)
    # The three methods of mfvit.attribution for the score of attention_relevance, y_t = (fused + x_cxr + x_enh)[t] (MAIN_CA:868), along the JOINT path
    # of both images: ((res_cxr, res_enh), stream_share).  baselines = (baseline_cxr, baseline_enh), each as integrated_gradients takes it;
    # streams = 'both' | 'cxr' | 'enh': with one stream the other image stays at its input at every step (a plain evaluation forward) and its
    # result is None.  stream_share = total_cxr / (total_cxr + total_enh), (B,) float64 on the device, NaN where the denominator is 0; for
    # integrated gradients the results' delta is the completeness gap of both totals together.  The encoders run one after the other on the
    # caller's stream; each attributed one runs its data-gradient-only backward.  Same contract as attention_relevance and perturbation_test: no
    # p.grad, no gradient arena, training flags, feature caches and RNG states (but for one drawn seed) as they were.
    def _attribution(self, method, vit_cxr, vit_enh, img_cxr, img_enh, target, kw):
        from mfvit import attribution
        self._check_pair(vit_cxr, vit_enh, img_cxr, img_enh)

        def out_of(f_c, f_e):
            hc, he = self._plain_head(vit_cxr), self._plain_head(vit_enh)
            if hc is not None and he is not None and hc.out_features == self.num_classes == he.out_features:
                fused, x_c, x_e = FusionFn.apply(self._spec, f_c, f_e, hc.weight, hc.bias, he.weight, he.bias, *self._spec.live())
            else:
                fused, _, _ = FusionFn.apply(self._spec, f_c, f_e, None, None, None, None, *self._spec.live())
                x_c, x_e = vit_cxr.forward_head(f_c), vit_enh.forward_head(f_e)
            return fused + x_c + x_e
        return attribution.two_stream(method, (vit_cxr, vit_enh), (img_cxr, img_enh), out_of, self.num_classes, (self, vit_cxr, vit_enh),
                                      target=target, **kw)

    def integrated_gradients(self, vit_cxr, vit_enh, img_cxr, img_enh, target=None, baselines=(None, None), streams="both", steps=20,
                             rule="trapezoid", score="logit", sign="signed", noise=None, max_batch=None, return_pixels=False):
        """mfvit.attribution.integrated_gradients for the two-stream model: see above."""
        return self._attribution("integrated_gradients", vit_cxr, vit_enh, img_cxr, img_enh, target,
                                 dict(baselines=baselines, streams=streams, steps=steps, rule=rule, score=score, sign=sign, noise=noise,
                                      max_batch=max_batch, return_pixels=return_pixels))

    def smoothgrad(self, vit_cxr, vit_enh, img_cxr, img_enh, target=None, streams="both", noise_level=0.15, samples=25, squared=False, seed=None,
                   times_input=False, score="logit", sign="signed", max_batch=None, return_pixels=False):
        """mfvit.attribution.smoothgrad for the two-stream model (stream i draws its noise from seed + i): see above."""
        return self._attribution("smoothgrad", vit_cxr, vit_enh, img_cxr, img_enh, target,
                                 dict(streams=streams, noise_level=noise_level, samples=samples, squared=squared, seed=seed, times_input=times_input,
                                      score=score, sign=sign, max_batch=max_batch, return_pixels=return_pixels))

    def saliency(self, vit_cxr, vit_enh, img_cxr, img_enh, target=None, streams="both", times_input=False, score="logit", sign="signed",
                 max_batch=None, return_pixels=False):
        """mfvit.attribution.saliency for the two-stream model: see above."""
        return self._attribution("saliency", vit_cxr, vit_enh, img_cxr, img_enh, target,
                                 dict(streams=streams, times_input=times_input, score=score, sign=sign, max_batch=max_batch,
                                      return_pixels=return_pixels))
