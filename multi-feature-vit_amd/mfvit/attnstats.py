"""Per-head attention statistics of the ViT encoders (include/mfvit.h, mfvit_attention_stats; csrc/attention_maps.hip).

Mean attention distance of every head of every block is Dosovitskiy et al. 2021, Fig. 11, and the second half of Raghu et al. 2021: which
heads look locally and which globally.  Attention entropy, the mass the patches send to the cls token (an attention sink) and the mass a
token keeps on itself are the per-head summaries reported beside it.  STATS names the six numbers in the kernel's order.

The kernel recomputes the softmax probabilities of a block from the qkv tensor and log-sum-exp its attention forward left behind - the same
sequence as get_attention_maps, so the same bits - and reduces them in registers: the T x T maps never reach memory.  Every sum runs in a
fixed order, f32 along a row and double from the rows upward.  No CPU / eager fallback.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream

STATS = ("distance", "distance_renorm", "entropy", "cls_entropy", "cls_mass", "self_mass")      # MFVIT_ATTN_NSTAT = 6
_TAGS = (_lib.F32, _lib.BF16, _lib.BF16X3, _lib.F16, _lib.X3F16)


def attention_stats(qkv, lse, qkv_dtype, B, T, H, head_dim, grid, patch=16.0, nblk=1, strides=None):
    """mfvit_attention_stats on caller-owned tensors: (nblk, B, H, 6) float64, STATS along the last axis.

    qkv: block 0's [B][T][3][H][head_dim] tensor in the storage format of tag qkv_dtype (any torch dtype: only its address is used);
    lse: block 0's f32 [B][H][T] natural-log log-sum-exp, as mfvit_attention_fwd wrote it; grid = (gh, gw) with T = 1 + gh * gw; patch: the
    patch edge in pixels.  strides = (qkv bytes, lse bytes) between consecutive blocks (multiples of 16); the default is the dense stack
    (nblk = 1: no stride is used)."""
    _lib.require_cuda(qkv, lse)
    if lse.dtype != torch.float32:
        raise ValueError(f"lse must be float32, got {lse.dtype}")
    if qkv_dtype not in _TAGS:
        raise ValueError(f"unknown qkv storage tag {qkv_dtype!r}")
    gh, gw = (int(g) for g in grid)
    nblk, B, T, H, head_dim = int(nblk), int(B), int(T), int(H), int(head_dim)
    if strides is None and nblk == 1:
        strides = (0, 0)
    elif strides is None:
        es = {_lib.F32: 4, _lib.BF16: 2, _lib.F16: 2, _lib.BF16X3: 4, _lib.X3F16: 4}[qkv_dtype]
        strides = (B * T * 3 * H * head_dim * es, B * H * T * 4)
    nbytes = lib().mfvit_attention_stats_work_bytes(nblk, B, T, H)
    if nbytes == 0:
        raise ValueError(f"invalid attention-statistics shape: nblk {nblk}, B {B}, T {T}, H {H}")
    work = torch.empty(nbytes, device=qkv.device, dtype=torch.uint8)
    out = torch.empty(nblk, B, H, len(STATS), device=qkv.device, dtype=torch.float64)
    check(lib().mfvit_attention_stats(qkv_dtype, ptr(qkv), ptr(lse), int(strides[0]), int(strides[1]), nblk, B, T, H, head_dim, gh, gw,
                                      float(patch), ptr(out), ptr(work), nbytes, stream()), "mfvit_attention_stats")
    return out


class AttentionStatsMeter:
    """Per-image means of the statistics over an epoch, accumulated on the device.

    update(stats): an (nblk, B, heads, 6) float64 GPU tensor (attention_stats' result); its sum over the images and the image count are added to
    device accumulators, nothing synchronises with the host.  result(): one copy to the host; {name: (nblk, heads) float64 array}."""

    def __init__(self, nblk, heads):
        if nblk < 1 or heads < 1:
            raise ValueError(f"nblk and heads must be positive, got {nblk} and {heads}")
        self.nblk, self.heads = int(nblk), int(heads)
        self._acc = None
        self.batches = 0

    def update(self, stats):
        _lib.require_cuda(stats)
        if stats.dim() != 4 or stats.dtype != torch.float64 or (stats.shape[0], stats.shape[2], stats.shape[3]) != (self.nblk, self.heads, len(STATS)):
            raise ValueError(f"expected a ({self.nblk}, B, {self.heads}, {len(STATS)}) float64 tensor, got {tuple(stats.shape)} {stats.dtype}")
        n = self.nblk * self.heads * len(STATS)
        if self._acc is None:
            self._acc = torch.zeros(n + 1, device=stats.device, dtype=torch.float64)
        self._acc[:n] += stats.sum(dim=1).reshape(-1)
        self._acc[n] += stats.shape[1]
        self.batches += 1

    def result(self):
        if self._acc is None:
            raise RuntimeError("AttentionStatsMeter.result() before any update()")
        a = self._acc.cpu().numpy()
        mean = (a[:-1] / a[-1]).reshape(self.nblk, self.heads, len(STATS))
        return {name: np.ascontiguousarray(mean[:, :, i]) for i, name in enumerate(STATS)}
