"""nn.CrossEntropyLoss (mean) for a handful of classes on the HIP path (MAIN_CA:432,873; MAIN_SS:714)."""
import torch

from . import ops


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss, dlogits, preds = ops.cross_entropy(logits.contiguous().float(), target.contiguous().long(), want_grad=True)
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(preds)
        return loss.reshape(()), preds

    @staticmethod
    def backward(ctx, gloss, _gpreds):
        (dlogits,) = ctx.saved_tensors
        return dlogits * gloss, None


def cross_entropy(logits, target):
    """Returns (loss scalar, preds) - preds = argmax(logits, 1) as torch.max would give (MAIN_CA:870)."""
    return _CEFn.apply(logits, target)


class _SoftCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, partner, lam, smoothing):
        loss, dlogits, preds = ops.cross_entropy_soft(logits.contiguous().float(), target, partner, lam, smoothing, want_grad=True)
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(preds)
        return loss.reshape(()), preds

    @staticmethod
    def backward(ctx, gloss, _gpreds):
        (dlogits,) = ctx.saved_tensors
        return dlogits * gloss, None, None, None, None


def soft_cross_entropy(logits, target, smoothing=None):
    """Soft-target cross entropy (mean) of a mixed batch: `target` is the MixTarget that mfvit.mixup.Mixup returned (its smoothing holds unless
    `smoothing` is given), or a plain int64 tensor - then this is nn.CrossEntropyLoss(label_smoothing=smoothing).  Returns (loss scalar,
    preds) like cross_entropy; the (B, C) soft labels are never built."""
    from .mixup import MixTarget
    if not isinstance(target, MixTarget):
        target = MixTarget(target, smoothing=0.0 if smoothing is None else smoothing)
    s = target.smoothing if smoothing is None else float(smoothing)
    if not 0.0 <= s < 1.0:
        raise ValueError(f"smoothing must lie in [0, 1), got {s}")
    if logits.dim() != 2 or target.target.shape != (logits.shape[0],):
        raise ValueError(f"soft_cross_entropy: logits [B][C] and target [B] disagree: {tuple(logits.shape)} and {tuple(target.target.shape)}")
    partner, lam = target.partner, target.lam
    if partner is not None:
        partner, lam = partner.contiguous().int(), lam.contiguous().float()
    return _SoftCEFn.apply(logits, target.target.contiguous().long(), partner, lam, s)
