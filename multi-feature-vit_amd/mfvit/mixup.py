"""Mixup / CutMix / random erasing for one batch or for the paired streams of the two-stream model, and the mixed target they produce.

The rest of the DeiT / MoCo-v3 fine-tune recipe next to the encoders' drop_path_rate: ``Mixup`` draws, on the host, one table row per
sample (mixing partner, mode, cut box, erase box) and one coefficient, and ONE launch of mfvit_batch_mix (csrc/mix.hip) erases and mixes the
batch - and its twin with the SAME partner, coefficient and boxes, so that a mixed (CXR, enhanced) pair still shows one patient.  The labels
travel as a ``MixTarget`` (target, partner, lam, smoothing) that ``mfvit.losses.soft_cross_entropy`` consumes without ever building the
(B, C) soft label matrix.

Definition.  timm is neither a dependency of this project nor part of the reference it was modelled on, so the sampler below is the project's
own statement of ``timm.data.Mixup`` / ``timm.data.RandomErasing(mode='const')``, written from their documented behaviour:
  * both alphas positive: CutMix with probability switch_prob, else Mixup; lam ~ Beta(alpha, alpha) of the chosen kind (two gamma draws
    g1 / (g1 + g2), which a torch.Generator determines); with probability 1 - prob no mixing (lam = 1, mode 0).
  * CutMix box: ratio = sqrt(1 - lam), cut_h, cut_w = int(H ratio), int(W ratio), centre cy ~ randint(0, H), cx ~ randint(0, W), edges clipped
    to the image; correct_lam: lam := 1 - box_area / (H W).
  * mode 'batch': one draw for the batch, 'elem': one per sample, 'pair': one per pair (i, n - 1 - i), shared by both halves.
  * partner 'flip': j = n - 1 - i (timm's x.flip(0)); 'perm': a random permutation.
  * erasing: per sample with probability erase_prob, up to 10 tries of area * U(erase_scale) at a log-uniform aspect ratio (as
    GpuTransform.resized_crop_box draws its crop), no box when none fits; the box is filled with 0, the dataset mean after Normalize.
    Erasing belongs to the loader, i.e. it comes BEFORE the mix: a sample is erased with its own box wherever it is read, as the partner too.
Order of the draws (every one from the generator): the permutation, then per draw unit [mix?, cutmix?, gamma pair, cy, cx], then per sample
[erase?, (area, aspect) x tries, top, left].
"""
import math

import torch

from . import _lib, ops

DESC_COLS = 12
MODE_COPY, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2


class MixTarget:
    """The label of a mixed batch: y_i = lam_i s(t_i) + (1 - lam_i) s(t_partner_i), s(t) = (1 - smoothing) onehot(t) + smoothing / C (timm's
    mixup_target).  target int64 [B]; partner int32 [B] and lam f32 [B] together, or both None (a plain hard target)."""

    def __init__(self, target, partner=None, lam=None, smoothing=0.0):
        if (partner is None) != (lam is None):
            raise ValueError("MixTarget: partner and lam come together")
        if not 0.0 <= float(smoothing) < 1.0:
            raise ValueError(f"smoothing must lie in [0, 1), got {smoothing}")
        self.target, self.partner, self.lam, self.smoothing = target, partner, lam, float(smoothing)

    def dense(self, num_classes):
        """The (B, C) f32 soft label matrix, for users who want timm's form (plain torch; the loss itself never builds it)."""
        t = self.target.long()
        if t.numel() and int(t.max()) >= num_classes:
            raise ValueError(f"num_classes = {num_classes} is smaller than max(target) + 1 = {int(t.max()) + 1}")
        off, on = self.smoothing / num_classes, 1.0 - self.smoothing
        s = torch.full((t.numel(), num_classes), off, dtype=torch.float64, device=t.device)
        s.scatter_add_(1, t[:, None], torch.full((t.numel(), 1), on, dtype=torch.float64, device=t.device))
        if self.partner is None:
            return s.float()
        lam = self.lam.double()[:, None]
        return (lam * s + (1.0 - lam) * s[self.partner.long()]).float()


def check_params(desc, lam, n, H, W):
    """The caller's contract of mfvit_batch_mix, on the host tables: partner in [0, n), mode in {0, 1, 2}, boxes ordered and inside the
    image, lam in [0, 1].  Raises ValueError."""
    if desc.shape != (n, DESC_COLS) or desc.dtype != torch.int32 or lam.shape != (n,) or lam.dtype != torch.float32:
        raise ValueError(f"mix tables must be int32 [{n}][{DESC_COLS}] and f32 [{n}], got {tuple(desc.shape)} {desc.dtype} and {tuple(lam.shape)} {lam.dtype}")
    d = desc.cpu()
    if n and (int(d[:, 0].min()) < 0 or int(d[:, 0].max()) >= n):
        raise ValueError(f"desc out of range: partner index outside [0, {n})")
    if n and (int(d[:, 1].min()) < 0 or int(d[:, 1].max()) > 2):
        raise ValueError("desc out of range: mode must be 0 (copy), 1 (mixup) or 2 (cutmix)")
    for c0, what in ((2, "cut"), (7, "erase")):
        lo_y, hi_y, lo_x, hi_x = (d[:, c0 + k] for k in range(4))
        if bool(((lo_y < 0) | (lo_y > hi_y) | (hi_y > H) | (lo_x < 0) | (lo_x > hi_x) | (hi_x > W)).any()):
            raise ValueError(f"desc out of range: a {what} box is not 0 <= lo <= hi <= ({H}, {W})")
    l = lam.cpu()
    if bool(((l < 0) | (l > 1) | l.isnan()).any()):
        raise ValueError("lam outside [0, 1]")


class Mixup(torch.nn.Module):
    """Mixup / CutMix / random erasing of a batch (or of the two streams of a pair) on the GPU; see the module docstring for the definition.

        mix = Mixup(label_smoothing=0.1, num_classes=3, erase_prob=0.25)
        x, xe, y = mix(x, target, xe)                       # one launch; y is a MixTarget
        loss, preds = soft_cross_entropy(logits, y)

    train() / eval() switch it like any module; in eval mode, or with enabled=False, it returns its inputs and a plain hard target."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", correct_lam=True, label_smoothing=0.1,
                 num_classes=3, partner="flip", erase_prob=0.0, erase_scale=(0.02, 1 / 3), erase_ratio=(0.3, 3.3), enabled=True):
        super().__init__()
        if mode not in ("batch", "elem", "pair"):
            raise ValueError(f"mode must be 'batch', 'elem' or 'pair', got {mode!r}")
        if partner not in ("flip", "perm"):
            raise ValueError(f"partner must be 'flip' or 'perm', got {partner!r}")
        if mode == "pair" and partner != "flip":
            raise ValueError("mode='pair' shares a draw between i and n - 1 - i: it needs partner='flip'")
        if mixup_alpha < 0 or cutmix_alpha < 0 or not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0 or not 0.0 <= erase_prob <= 1.0:
            raise ValueError("alphas must be >= 0 and prob, switch_prob, erase_prob probabilities")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing}")
        if not (0.0 < erase_scale[0] <= erase_scale[1] <= 1.0 and 0.0 < erase_ratio[0] <= erase_ratio[1]):
            raise ValueError("erase_scale must be 0 < lo <= hi <= 1 and erase_ratio 0 < lo <= hi")
        if num_classes < 1:
            raise ValueError("num_classes must be positive")
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob)
        self.mode, self.correct_lam, self.label_smoothing, self.num_classes, self.partner = mode, bool(correct_lam), float(label_smoothing), int(num_classes), partner
        self.erase_prob, self.erase_scale, self.erase_ratio = float(erase_prob), (float(erase_scale[0]), float(erase_scale[1])), (float(erase_ratio[0]), float(erase_ratio[1]))
        self.enabled = bool(enabled)

    # ------------------------------------------------------------------------------------------------ host-side sampling
    @staticmethod
    def _rand(g):
        return float(torch.rand(1, dtype=torch.float64, generator=g))

    def _draw_mix(self, H, W, g):
        """One draw unit: (mode, lam as f64, (yl, yh, xl, xh))."""
        if (self.mixup_alpha <= 0 and self.cutmix_alpha <= 0) or not self._rand(g) < self.prob:
            return MODE_COPY, 1.0, (0, 0, 0, 0)
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cutmix = self._rand(g) < self.switch_prob
        else:
            cutmix = self.cutmix_alpha > 0
        alpha = self.cutmix_alpha if cutmix else self.mixup_alpha
        g1, g2 = torch._standard_gamma(torch.tensor([alpha, alpha], dtype=torch.float64), generator=g).tolist()
        lam = g1 / (g1 + g2) if g1 + g2 > 0 else 0.5      # (both gammas underflow only for alpha far below any recipe's)
        lam = min(max(lam, 0.0), 1.0)
        if not cutmix:
            return MODE_MIXUP, lam, (0, 0, 0, 0)
        ratio = math.sqrt(1.0 - lam)
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy, cx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
        yl, yh = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
        xl, xh = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
        if self.correct_lam:
            lam = 1.0 - ((yh - yl) * (xh - xl)) / float(H * W)
        return MODE_CUTMIX, lam, (yl, yh, xl, xh)

    def _draw_erase(self, H, W, g):
        """(eyl, eyh, exl, exh) of one sample, or None."""
        if self.erase_prob <= 0 or not self._rand(g) < self.erase_prob:
            return None
        area = H * W
        lo, hi = math.log(self.erase_ratio[0]), math.log(self.erase_ratio[1])
        for _ in range(10):
            target_area = area * float(torch.empty(1, dtype=torch.float64).uniform_(self.erase_scale[0], self.erase_scale[1], generator=g))
            aspect = math.exp(float(torch.empty(1, dtype=torch.float64).uniform_(lo, hi, generator=g)))
            h, w = int(round(math.sqrt(target_area * aspect))), int(round(math.sqrt(target_area / aspect)))
            if 0 < h < H and 0 < w < W:
                top = int(torch.randint(0, H - h + 1, (1,), generator=g))
                left = int(torch.randint(0, W - w + 1, (1,), generator=g))
                return top, top + h, left, left + w
        return None

    def sample_params(self, n, H, W, generator=None):
        """The random draws of one batch of n images of H x W: CPU tensors desc (int32 [n][12], the table of mfvit_batch_mix) and lam
        (f32 [n]).  Pure host code; every draw comes from `generator`, so a seed reproduces the tables."""
        if n < 1 or H < 1 or W < 1:
            raise ValueError("sample_params needs n, H, W >= 1")
        g = generator
        desc = torch.zeros(n, DESC_COLS, dtype=torch.int32)
        lam = torch.ones(n, dtype=torch.float64)
        desc[:, 0] = torch.randperm(n, generator=g).int() if self.partner == "perm" else torch.arange(n - 1, -1, -1, dtype=torch.int32)
        if self.mode == "batch":
            units = [range(n)]
        elif self.mode == "elem":
            units = [(i,) for i in range(n)]
        else:
            units = [(i, n - 1 - i) if i != n - 1 - i else (i,) for i in range((n + 1) // 2)]
        for unit in units:
            mode, l, box = self._draw_mix(H, W, g)
            for i in unit:
                desc[i, 1] = mode
                desc[i, 2:6] = torch.tensor(box, dtype=torch.int32)
                lam[i] = l
        for i in range(n):
            box = self._draw_erase(H, W, g)
            if box is not None:
                desc[i, 6] = 1
                desc[i, 7:11] = torch.tensor(box, dtype=torch.int32)
        return desc, lam.float()

    # ------------------------------------------------------------------------------------------------ the device side
    def forward(self, x, target, x2=None, params=None, generator=None):
        """x (and x2, its twin): f32 NCHW on the device; target: int64 [n] (on either side).  Returns (x_mixed, mix_target), or
        (x_mixed, x2_mixed, mix_target) with x2.  params = (desc, lam) replays given tables (CPU or device tensors) instead of drawing.
        The mixed batch is new data, not an autograd node: an input with requires_grad is refused (image gradients are then taken with respect
        to the MIXED image, which is what FGSM on a mixed batch means)."""
        if x.requires_grad or (x2 is not None and x2.requires_grad):
            raise ValueError("Mixup: the mixed batch is new data, not an autograd node - detach the input (and take image gradients of the mixed batch)")
        if x.dim() != 4:
            raise ValueError(f"Mixup: the batch must be NCHW, got {tuple(x.shape)}")
        if x2 is not None and x2.shape != x.shape:
            raise ValueError(f"Mixup: the two streams differ in shape: {tuple(x.shape)} and {tuple(x2.shape)}")
        n, _, H, W = x.shape
        if target.shape != (n,) or target.dtype != torch.int64:
            raise ValueError(f"Mixup: target must be int64 [{n}], got {target.dtype} {tuple(target.shape)}")
        if not self.training or not self.enabled:
            y = MixTarget(target.to(x.device))
            return (x, y) if x2 is None else (x, x2, y)
        if n and int(target.max()) >= self.num_classes:      # (synchronises when the labels already live on the device)
            raise ValueError(f"Mixup: num_classes = {self.num_classes} is smaller than max(target) + 1 = {int(target.max()) + 1}")
        desc, lam = self.sample_params(n, H, W, generator) if params is None else params
        check_params(desc, lam, n, H, W)
        _lib.require_cuda(x, x2)
        desc, lam = desc.to(x.device).contiguous(), lam.to(x.device).contiguous()
        xa = x.float().contiguous()
        y = MixTarget(target.to(x.device).contiguous(), desc[:, 0].contiguous(), lam, self.label_smoothing)
        if x2 is None:
            return ops.batch_mix(xa, desc, lam), y
        out_a, out_b = ops.batch_mix(xa, desc, lam, x2.float().contiguous())
        return out_a, out_b, y
