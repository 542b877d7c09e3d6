"""ctypes binding of libmfvit_hip.so (C ABI declared in include/mfvit.h).

The product path has NO CPU / eager fallback: if the HIP library is missing, cannot be loaded, or an op is asked
to run on a non-GPU tensor, a RuntimeError is raised.
"""
import ctypes
import os

import torch  # noqa: F401  MUST precede loading libmfvit_hip.so: torch bundles its own libamdhip64.so.7 / libhsa-runtime64;
#                      whichever copy of that SONAME is mapped first serves the whole process, and mixing the system
#                      runtime with torch's bundled HSA layer leaves the extension with "no ROCm-capable device"
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFVIT_LIB") or os.path.join(_HERE, "libmfvit_hip.so")   # MFVIT_LIB: experiment builds
ABI_VERSION = 5   # mfvit_abi_version() of the library the ctypes structs below are written for (include/mfvit.h)

F32, BF16, BF16X3, F16, X3F16 = 0, 1, 2, 3, 4   # X3F16: split fp16, the qkv operand of the attention core in bf16x3 mode
EPI_BIAS, EPI_BIAS_GELU, EPI_NONE, EPI_BIAS_X3F16 = 0, 1, 3, 5


class VitCfg(Structure):
    _fields_ = [("dtype", c_int), ("batch", c_int), ("img_h", c_int), ("img_w", c_int), ("dim", c_int), ("depth", c_int),
                ("heads", c_int), ("mlp_dim", c_int), ("save_for_backward", c_int), ("stop_grad_conv1", c_int),
                ("ln_eps", c_float), ("token_input", c_int), ("tokens", c_int), ("use_pos", c_int), ("act", c_int),
                ("p_embd", c_float), ("p_attn", c_float), ("p_resid", c_float), ("seed_lo", c_uint32), ("seed_hi", c_uint32),
                ("stream_share", c_int)]


class VitDrop(Structure):
    """mfvit_vit_drop: training-mode dropout / drop-path rates of the image encoder (include/mfvit.h)."""
    _fields_ = [("drop", c_float), ("attn_drop", c_float), ("drop_path", POINTER(c_float)), ("seed", c_uint64)]


class PatchKeepCfg(Structure):
    """mfvit_patch_keep_cfg: the patch-dropout front end's shape (include/mfvit.h; timm PatchDropout)."""
    _fields_ = [("dtype", c_int), ("batch", c_int), ("img_h", c_int), ("img_w", c_int), ("keep", c_int), ("dim", c_int)]


class VitSeg(Structure):
    """mfvit_vit_seg: a block range of the image-mode stack at a given sequence length (include/mfvit.h)."""
    _fields_ = [("block_lo", c_int), ("block_hi", c_int), ("tokens", c_int), ("image_in", c_int)]


class VitAttnReq(Structure):
    """mfvit_vit_attn_req: which attention maps / rollout an evaluation forward writes (include/mfvit.h)."""
    _fields_ = [("blocks", c_uint64), ("fuse", c_int), ("cls_only", c_int), ("maps", c_void_p), ("rollout", c_void_p), ("scratch", c_void_p)]


HEAD_FUSION = {None: 0, "mean": 1, "max": 2, "min": 3}     # mfvit_vit_attn_req::fuse


class VitRelReq(Structure):
    """mfvit_vit_rel_req: which relevance maps / cls-row relevance a relevance backward writes (include/mfvit.h)."""
    _fields_ = [("blocks", c_uint64), ("maps", c_void_p), ("relevance", c_void_p), ("scratch", c_void_p)]


class LoraItem(Structure):
    """mfvit_lora_item: one (block, target) adapter pair of a request (include/mfvit.h)."""
    _fields_ = [("block", c_int), ("target", c_int), ("a", c_void_p), ("b", c_void_p), ("da", c_void_p), ("db", c_void_p)]


class LoraReq(Structure):
    """mfvit_lora_req: rank, scale and the host array of items."""
    _fields_ = [("rank", c_int), ("scale", c_float), ("n", c_int), ("items", POINTER(LoraItem))]


OPTIM_GROUPS_PER_LAUNCH = 64   # MFVIT_OPTIM_GROUPS_PER_LAUNCH: hyper entries one launch of the group-aware steps carries in its arguments


class AdamGroup(Structure):
    """mfvit_adam_group: the hyperparameters of one param group for mfvit_adam_step_groups (include/mfvit.h)."""
    _fields_ = [("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("step", ctypes.c_int32), ("decoupled", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SgdGroup(Structure):
    """mfvit_sgd_group: the hyperparameters of one param group for mfvit_sgd_step_groups (include/mfvit.h)."""
    _fields_ = [("lr", c_float), ("momentum", c_float), ("weight_decay", c_float), ("reserved", ctypes.c_int32)]


class FusionCfg(Structure):
    _fields_ = [("batch", c_int), ("tokens", c_int), ("dim", c_int), ("heads", c_int), ("num_classes", c_int),
                ("eps_pre", c_float), ("eps_post", c_float)]


P = c_void_p
I = c_int
L = c_int64
F = c_float
D = c_double

# name -> (restype, argtypes); must list every symbol of include/mfvit.h (tests/test_boundary_cpu.py checks it)
SIGNATURES = {
    "mfvit_abi_version": (I, []),
    "mfvit_build_info": (c_char_p, []),
    "mfvit_vit_param_count": (c_size_t, [POINTER(VitCfg)]),
    "mfvit_vit_param_layout": (I, [POINTER(VitCfg), POINTER(c_int64)]),
    "mfvit_vit_shadow_bytes": (c_size_t, [POINTER(VitCfg)]),
    "mfvit_vit_prepare_shadow": (I, [POINTER(VitCfg), P, P, P]),
    "mfvit_vit_workspace_bytes": (c_size_t, [POINTER(VitCfg)]),
    "mfvit_vit_forward": (I, [POINTER(VitCfg), P, P, P, P, P, P]),
    "mfvit_vit_backward": (I, [POINTER(VitCfg), P, P, P, P, P, I, I, P]),
    "mfvit_vit_workspace_bytes_drop": (c_size_t, [POINTER(VitCfg), POINTER(VitDrop)]),
    "mfvit_vit_forward_drop": (I, [POINTER(VitCfg), POINTER(VitDrop), P, P, P, P, P, P]),
    "mfvit_vit_backward_drop": (I, [POINTER(VitCfg), POINTER(VitDrop), P, P, P, P, P, I, I, P]),
    "mfvit_vit_workspace_bytes_ex": (c_size_t, [POINTER(VitCfg), POINTER(VitDrop), I]),
    "mfvit_vit_backward_ex": (I, [POINTER(VitCfg), POINTER(VitDrop), P, P, P, P, P, P, I, I, P]),
    "mfvit_vit_workspace_bytes_x0": (c_size_t, [POINTER(VitCfg), POINTER(VitDrop), I]),
    "mfvit_vit_forward_x0": (I, [POINTER(VitCfg), POINTER(VitDrop), I, P, P, P, P, P, P]),
    "mfvit_vit_backward_x0": (I, [POINTER(VitCfg), POINTER(VitDrop), I, P, P, P, P, P, P, I, I, P]),
    "mfvit_patch_keep_workspace_bytes": (c_size_t, [POINTER(PatchKeepCfg), I]),
    "mfvit_patch_keep_embed": (I, [POINTER(PatchKeepCfg), P, P, P, P, P, P, P, I, P, P, P]),
    "mfvit_patch_keep_embed_bwd": (I, [POINTER(PatchKeepCfg), P, P, P, P, P, P, P, P, P]),
    "mfvit_vit_workspace_bytes_seg": (c_size_t, [POINTER(VitCfg), POINTER(VitDrop), POINTER(VitSeg), I]),
    "mfvit_vit_attn_layout_seg": (I, [POINTER(VitCfg), POINTER(VitDrop), POINTER(VitSeg), POINTER(c_int64)]),
    "mfvit_vit_forward_seg": (I, [POINTER(VitCfg), POINTER(VitDrop), POINTER(VitSeg), P, P, P, P, P, P]),
    "mfvit_vit_backward_seg": (I, [POINTER(VitCfg), POINTER(VitDrop), POINTER(VitSeg), P, P, P, P, P, P, P, I, I, P]),
    "mfvit_vit_hidden_layout": (I, [POINTER(VitCfg), POINTER(c_int64)]),
    "mfvit_vit_attn_layout": (I, [POINTER(VitCfg), POINTER(c_int64)]),
    "mfvit_vit_attn_scratch_bytes": (c_size_t, [POINTER(VitCfg), POINTER(VitAttnReq)]),
    "mfvit_vit_forward_attn": (I, [POINTER(VitCfg), POINTER(VitAttnReq), P, P, P, P, P, P]),
    "mfvit_vit_rel_scratch_bytes": (c_size_t, [POINTER(VitCfg), POINTER(VitRelReq)]),
    "mfvit_vit_backward_rel": (I, [POINTER(VitCfg), POINTER(VitRelReq), P, P, P, P, P]),
    "mfvit_lora_merge": (I, [P, L, P, P, F, P, L, I, I, I, P]),
    "mfvit_lora_grad": (I, [P, L, P, P, F, P, P, I, I, I, P]),
    "mfvit_vit_prepare_shadow_lora": (I, [POINTER(VitCfg), P, POINTER(LoraReq), P, P, P]),
    "mfvit_vit_backward_lora": (I, [POINTER(VitCfg), POINTER(VitDrop), P, P, P, P, POINTER(LoraReq), P, P, I, I, P]),
    "mfvit_vit_lora_grad": (I, [POINTER(VitCfg), POINTER(LoraReq), P, P]),
    "mfvit_gpt_forward": (I, [POINTER(VitCfg), P, P, P, P, P, P]),
    "mfvit_gpt_backward": (I, [POINTER(VitCfg), P, P, P, P, P, P, P]),
    "mfvit_linear_fwd": (I, [I, I, P, L, P, L, P, P, L, P, L, I, I, I, P]),
    "mfvit_linear_dgrad_act": (I, [I, P, L, P, L, P, L, P, L, I, I, I, P]),
    "mfvit_linear_wgrad": (I, [I, P, L, P, L, P, L, I, I, I, P]),
    "mfvit_linear_wgrad_ws": (I, [I, P, L, P, L, P, L, I, I, I, P, P]),
    "mfvit_linear_wgrad_ex": (I, [I, P, L, P, L, P, L, I, I, I, P, P, I, I, I, P]),
    "mfvit_linear_wgrad_plan": (I, [I, I, I, I, I, L, L, L, L, L, L, I, POINTER(ctypes.c_int32)]),
    "mfvit_linear_wgrad_pair": (I, [I, P, L, P, L, P, L, P, I, P, L, P, L, P, L, I, I, I, P]),
    "mfvit_linear_res_ln_fwd": (I, [I, P, L, P, L, P, P, L, P, P, I, P, P, F, P, P, I, I, P]),
    "mfvit_linear_dgrad_ln_bwd": (I, [I, P, L, P, L, P, P, P, P, P, P, P, P, P, P, I, I, P]),
    "mfvit_linear_res_ln_fwd_ws": (I, [I, P, L, P, L, P, P, L, P, P, I, P, P, F, P, P, I, I, P, P]),
    "mfvit_linear_dgrad_ln_bwd_ws": (I, [I, P, L, P, L, P, P, P, P, P, P, P, P, P, P, I, I, P, P]),
    "mfvit_attention_fwd": (I, [I, P, P, P, I, I, I, I, P]),
    "mfvit_attention_bwd": (I, [I, P, P, P, P, P, P, I, I, I, I, P]),
    "mfvit_attention_qkv_dtype": (I, [I, I, I]),
    "mfvit_attention_plan": (I, [I, I, I, I, I, I, POINTER(ctypes.c_int32)]),
    "mfvit_attention_stats_work_bytes": (c_size_t, [I, I, I, I]),
    "mfvit_attention_stats": (I, [I, P, P, L, L, I, I, I, I, I, I, I, F, P, P, c_size_t, P]),
    "mfvit_attention_drop_fwd": (I, [I, P, P, P, I, I, I, I, F, c_uint64, c_uint32, P]),
    "mfvit_attention_drop_bwd": (I, [I, P, P, P, P, P, I, I, I, I, F, c_uint64, c_uint32, P]),
    "mfvit_dropout_mask": (I, [F, c_uint64, c_uint32, L, P, P]),
    "mfvit_layernorm_fwd": (I, [I, P, P, I, P, P, F, P, P, I, I, P]),
    "mfvit_layernorm_bwd": (I, [I, P, P, P, P, P, P, P, P, P, P, P, I, I, P]),
    "mfvit_cast_transpose": (I, [I, P, P, P, I, I, P]),
    "mfvit_head_fwd": (I, [P, L, P, P, P, L, I, I, I, I, P]),
    "mfvit_head_bwd": (I, [P, L, P, L, P, P, L, I, P, P, I, I, I, P]),
    "mfvit_cross_entropy": (I, [P, P, P, P, P, I, I, P]),
    "mfvit_cross_entropy_soft": (I, [P, P, P, P, F, P, P, P, I, I, P]),
    "mfvit_batch_mix": (I, [P, P, P, P, P, P, I, I, I, I, P]),
    "mfvit_fusion_param_count": (c_size_t, [POINTER(FusionCfg)]),
    "mfvit_fusion_workspace_bytes": (c_size_t, [POINTER(FusionCfg)]),
    "mfvit_fusion_forward": (I, [POINTER(FusionCfg), P, P, P, P, P, P, P, P, P, P, P, P]),
    "mfvit_fusion_ex_param_count": (c_size_t, [POINTER(FusionCfg), I, I]),
    "mfvit_fusion_ex_workspace_bytes": (c_size_t, [POINTER(FusionCfg), I, I]),
    "mfvit_fusion_ex_forward": (I, [POINTER(FusionCfg), I, I, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mfvit_fusion_ex_backward": (I, [POINTER(FusionCfg), I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mfvit_fusion_ex_attention": (I, [POINTER(FusionCfg), I, I, P, I, I, P, P]),
    "mfvit_fusion_ex_grad_attention": (I, [POINTER(FusionCfg), I, I, P, P, P, P, I, P, P]),
    "mfvit_bimodal_relevance_scratch_bytes": (c_size_t, [I, I]),
    "mfvit_bimodal_relevance": (I, [I, I, I, I, P, P, P, P, P, P]),
    "mfvit_bn_stats": (I, [I, P, I, I, P, P, P]),
    "mfvit_bn_combine": (I, [P, P, P, I, I, F, F, P, P, P, P, P]),
    "mfvit_bn_apply": (I, [I, P, P, P, P, P, I, P, I, I, P]),
    "mfvit_bn_bwd_sums": (I, [I, P, P, P, P, P, I, I, I, P, P, P]),
    "mfvit_bn_bwd_apply": (I, [I, P, P, P, P, P, P, I, P, P, F, P, I, I, P]),
    "mfvit_l2norm_fwd": (I, [P, P, P, I, I, F, P]),
    "mfvit_l2norm_bwd": (I, [P, P, P, P, I, I, P]),
    "mfvit_rowdot": (I, [P, P, P, L, F, I, I, P]),
    "mfvit_cross_entropy_rows": (I, [P, L, P, P, P, P, L, I, I, P]),
    "mfvit_ema_update": (I, [P, P, F, L, P]),
    "mfvit_lars_step": (I, [P, I, I, P, F, F, F, F, P]),
    "mfvit_adam_step": (I, [P, I, F, F, F, F, F, I, P]),
    "mfvit_sgd_step": (I, [P, I, F, F, F, I, P]),
    "mfvit_adam_step_groups": (I, [P, I, P, I, P]),
    "mfvit_sgd_step_groups": (I, [P, I, P, I, P]),
    "mfvit_amp_unscale": (I, [P, I, F, P, P]),
    "mfvit_grad_norm_partials": (I, [P, I, I, P, P]),
    "mfvit_grad_clip_coef": (I, [P, P, I, I, I, D, P, P, P]),
    "mfvit_grad_scale": (I, [P, I, P, P]),
    "mfvit_sam_norm_partials": (I, [P, I, I, P, P]),
    "mfvit_sam_scale": (I, [P, I, P, P, P]),
    "mfvit_sam_perturb": (I, [P, I, P, F, P]),
    "mfvit_sam_restore": (I, [P, I, P, P]),
    "mfvit_prenorm_xattn_forward": (I, [POINTER(FusionCfg), P, P, P, P, P, P]),
    "mfvit_prenorm_xattn_backward": (I, [POINTER(FusionCfg), P, P, P, P, P, P, P, P, P]),
    "mfvit_xattn_forward": (I, [POINTER(FusionCfg), P, P, P, P, P]),
    "mfvit_xattn_backward": (I, [POINTER(FusionCfg), P, P, P, P, P, P, P]),
    "mfvit_input_transform": (I, [P, P, P, I, I, I, P, P, P, P]),
    "mfvit_input_transform_rect": (I, [P, P, P, I, I, I, I, P, P, P, P]),
    "mfvit_input_photometric_workspace_bytes": (c_size_t, [I, I]),
    "mfvit_input_photometric": (I, [P, P, P, P, I, I, I, P, P, P, P, P]),
    "mfvit_eval_counts": (I, [P, L, P, I, I, P, P, P, P, P]),
    "mfvit_boot_work_bytes": (c_size_t, [I, I, I, L]),
    "mfvit_boot_counts": (I, [P, L, L, P, I, I, I, c_uint64, L, L, I, P, c_size_t, P, P, P, P]),
    "mfvit_delong_counts": (I, [P, L, L, P, I, I, I, P, c_size_t, P, P, P, P, P, P]),
    "mfvit_curve_counts": (I, [P, L, L, P, I, I, I, P, c_size_t, P, P, P, P, P, P, P]),
    "mfvit_boot_points": (I, [P, L, L, P, I, I, I, c_uint64, L, L, I, P, I, P, c_size_t, P, P, P, P, P]),
    "mfvit_calib_sums": (I, [P, L, L, P, I, I, I, P, I, I, P, P, P, P, P, P]),
    "mfvit_gram_plan": (I, [I, L, POINTER(ctypes.c_int32)]),
    "mfvit_gram_work_bytes": (c_size_t, [I, I, L]),
    "mfvit_gram_centered": (I, [P, L, L, I, I, L, P, P, c_size_t, P]),
    "mfvit_hsic_accumulate": (I, [P, I, P, I, I, I, P, P, P, P]),
    "mfvit_patch_rank": (I, [P, L, P, I, I, P]),
    "mfvit_patch_perturb": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "mfvit_perturb_score": (I, [P, L, P, I, I, I, P, P, P, P]),
    "mfvit_attr_inputs": (I, [P, P, I, P, P, P, I, P, I, I, I, L, P]),
    "mfvit_attr_accumulate": (I, [P, P, P, I, I, L, I, P]),
    "mfvit_attr_finish": (I, [P, P, P, I, I, I, P, P, P, I, I, I, I, P]),
    "mfvit_token_score": (I, [I, P, P, I, I, I, I, P, P, P]),
    "mfvit_token_select": (I, [P, L, I, I, I, P, P, P, P, P, P]),
    "mfvit_token_reorg_fwd": (I, [P, P, P, P, P, I, I, I, I, I, P, P]),
    "mfvit_token_reorg_bwd": (I, [P, P, P, P, P, I, I, I, I, I, P, P]),
    "mfvit_prof_enable": (I, [I]),
    "mfvit_set_wgrad_stream": (I, [I]),
    "mfvit_set_stream_share": (I, [I]),
    "mfvit_prof_collect": (I, [POINTER(ctypes.c_double), I]),
    "mfvit_prof_collect_tags": (I, [POINTER(ctypes.c_double), I]),
    "mfvit_prof_class_name": (c_char_p, [I]),
    "mfvit_fusion_backward": (I, [POINTER(FusionCfg), P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
}

_lib = None


class MfvitError(RuntimeError):
    pass


def lib():
    """Load (once) and return the HIP library; raise loudly when it is absent or built for another C ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MfvitError(
            f"libmfvit_hip.so not found at {LIB_PATH}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU/eager fallback for the MF-ViT hot path.")
    try:
        h = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime etc.
        raise MfvitError(f"cannot load {LIB_PATH}: {e}") from e
    abi = h.mfvit_abi_version()
    if abi != ABI_VERSION:   # (an older variant build through MFVIT_LIB: its structs differ from the ones passed here)
        raise MfvitError(f"{LIB_PATH} has C ABI {abi}, this package expects ABI {ABI_VERSION}: rebuild the library")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(h, name)
        fn.restype = res
        fn.argtypes = args
    _lib = h
    return h


def source_hash():
    """sha1 over the kernel sources (csrc/*.hip, *.cuh, *.h + include/mfvit.h): stamps measurements (PMC traffic files under
    profiles/) with the code they were taken on, so that bench.py never reports a figure measured on other kernels."""
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cuh", ".h")))
    files.append(os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "mfvit.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def check(rc, what):
    if rc != 0:
        raise MfvitError(f"{what} failed with code {rc} (-22 = invalid argument, -5 = launch error, -38 = not built for this dtype / size)")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MfvitError("MF-ViT HIP ops need tensors on a ROCm GPU ('cuda' device); there is no CPU fallback")


PRECISIONS = ("bf16x3", "bf16", "fp16", "fp32")


def dtype_code(precision):
    """'bf16x3' = split bf16 (three bf16 MFMAs per product: f32-grade results, meets the 1e-3 logits gate); 'bf16' = throughput mode;
    'fp16' = the reference's autocast arithmetic (pair with mfvit.amp.GradScaler); 'fp32' = exact f32 MFMA."""
    if precision in ("bf16x3", "split", "split-bf16"):
        return BF16X3
    if precision in ("bf16", "bfloat16"):
        return BF16
    if precision in ("fp16", "f16", "float16", "half"):
        return F16
    if precision in ("fp32", "f32", "float32"):
        return F32
    raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
