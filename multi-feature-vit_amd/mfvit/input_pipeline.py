"""GPU-side input pipeline: the finetune transform chain of aihc_utils/image_transform.py:50-84 as one HIP kernel.

    tf = GpuTransform(img_type="CheXpert-v1.0-small", img_size=256, crop=224, rotate=10, training=True, maintain_ratio=True)
    batch = tf(list_of_uint8_HWC_arrays)            # float32 [B, 3, 224, 224] on the GPU, what the DataLoader used to deliver
    q, k = tf.two_views(list_of_uint8_HWC_arrays)   # MoCo: two random views of each image (moco/loader.py:121-137)

The DataLoader workers then only decode (cv2.imread, moco/loader.py:121) and hand over uint8 HWC arrays of any size; Resize((S,S))
or Resize(S) (maintain_ratio: shorter side S) -> RandomHorizontalFlip -> RandomRotation(rotate) -> RandomCrop((crop,crop)) |
CenterCrop -> ToTensor -> Normalize run fused on the device, bit-exact against Pillow's integer arithmetic (the backend
torchvision's PIL transforms call).  This module is the host half: the per-axis fixed-point coefficient tables and the 16.16
affine terms, computed in double exactly as Pillow does.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream

# per-dataset statistics, image_transform.py:4-19
NORMALIZE = {
    "CheXpert-v1.0-small": ([.5020, .5020, .5020], [float(np.round(np.sqrt(.085585), 4))] * 3),
    "CheXpert_Enh": ([.6086, .5204, .3384], [.134909, .088268, .035044]),
    "data": ([0.5045, 0.5045, 0.5045], [0.2462, 0.2462, 0.2462]),
    "Train_Mix": ([0.2243, 0.5507, 0.6865], [0.1026, 0.2995, 0.3300]),
}
_PREC = 32 - 8 - 2
_AXIS_CACHE = {}


def axis_table(in_size, out_size):
    """int32 [out_size][2 + ksize]: first source index, tap count, taps - Pillow's precompute_coeffs + normalize_coeffs_8bpc for
    the triangle (BILINEAR) filter stretched by max(scale, 1) (antialiasing on downscale)."""
    key = (in_size, out_size)
    if key in _AXIS_CACHE:
        return _AXIS_CACHE[key]
    scale = float(in_size) / out_size
    fscale = scale if scale > 1.0 else 1.0
    support = fscale
    ksize = int(math.ceil(support)) * 2 + 1
    tab = np.zeros((out_size, 2 + ksize), dtype=np.int32)
    inv = 1.0 / fscale
    for o in range(out_size):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        taps, total = [], 0.0
        for t in range(n):
            u = abs((t + lo - center + 0.5) * inv)
            wgt = 1.0 - u if u < 1.0 else 0.0
            taps.append(wgt)
            total += wgt
        tab[o, 0], tab[o, 1] = lo, n
        for t in range(n):
            v = taps[t] / total if total != 0.0 else taps[t]
            tab[o, 2 + t] = int(v * (1 << _PREC) - 0.5) if v < 0 else int(v * (1 << _PREC) + 0.5)
    _AXIS_CACHE[key] = (ksize, tab)
    return ksize, tab


def resized_size(h, w, size):
    """(h, w) of transforms.Resize(size) with an int size (torchvision's _compute_resized_output_size): the shorter side becomes
    `size`, the longer int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def rotation_terms(angle, w, h=None):
    """(mode, a0..a5): Image.rotate(angle, NEAREST, expand=False) on a w x h image (h defaults to w).  mode 0 none, 1 affine
    (16.16 fixed-point terms of libImaging's affine_fixed), 2/3/4 the transpose fast paths for 90/180/270 degrees - which Pillow
    takes for 90 and 270 only on a square image."""
    h = w if h is None else h
    angle = angle % 360.0
    if angle == 0:
        return 0, (0,) * 6
    if angle == 180 or (angle in (90, 270) and w == h):
        return {90: 2, 180: 3, 270: 4}[int(angle)], (0,) * 6
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2] + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5] + cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return 1, (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


class GpuTransform:
    """Mirror of `get_transform_type(args, training, img_type)` (image_transform.py:50-84): args.img_size -> img_size, args.crop ->
    crop (0 = no crop), args.rotate -> rotate (degrees; RandomRotation draws from [-rotate, rotate]), args.maintain_ratio ->
    maintain_ratio (False: Resize((S, S)) squashes every image to a square; True: Resize(S), the shorter side becomes S and the
    aspect ratio is kept)."""

    def __init__(self, img_type="CheXpert-v1.0-small", img_size=256, crop=224, rotate=10, training=True, device="cuda:0",
                 mocov3=False, crop_min=0.08, maintain_ratio=False):
        """mocov3=True mirrors `get_transform_type_mocov3` (image_transform.py:86-124, MoCo pretraining): training =
        RandomResizedCrop(img_size, scale=(crop_min, 1)) -> flip -> rotation (no further crop; maintain_ratio has no effect);
        evaluation = Resize((256, 256)) | Resize(256) (maintain_ratio) -> CenterCrop(crop)."""
        self.mocov3, self.crop_min = bool(mocov3), float(crop_min)
        if mocov3:
            if training:
                crop = 0
            else:
                img_size = 256
        if img_type not in NORMALIZE:
            raise _lib.MfvitError(f"unknown img_type {img_type!r} (image_transform.py:72-81 knows {sorted(NORMALIZE)})")
        self.mean, self.std = NORMALIZE[img_type]
        self.size, self.crop, self.rotate, self.training = int(img_size), int(crop) if crop else int(img_size), float(rotate), training
        self.no_crop = not crop
        # the resized frame follows the image's aspect ratio (RandomResizedCrop's output is square whatever the flag says)
        self.maintain_ratio = bool(maintain_ratio) and not (self.mocov3 and training)
        if self.crop > self.size:
            raise _lib.MfvitError("crop larger than the resized image")
        self.device = torch.device(device)

    def frame(self, h, w):
        """(Sh, Sw): the resized frame of an h x w source (window)."""
        return resized_size(h, w, self.size) if self.maintain_ratio else (self.size, self.size)

    @staticmethod
    def resized_crop_box(height, width, scale, generator=None, ratio=(3.0 / 4.0, 4.0 / 3.0)):
        """torchvision RandomResizedCrop.get_params: (i, j, h, w) of the source window (10 tries, then the central fallback)."""
        area = height * width
        log_ratio = torch.log(torch.tensor(ratio))
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
            aspect = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=generator)).item()
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= width and 0 < h <= height:
                i = int(torch.randint(0, height - h + 1, (1,), generator=generator))
                j = int(torch.randint(0, width - w + 1, (1,), generator=generator))
                return i, j, h, w
        in_ratio = float(width) / float(height)
        if in_ratio < min(ratio):
            w = width
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = height
            w = int(round(h * max(ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def sample_params(self, n, generator=None, sizes=None):
        """The random draws of one batch, in torchvision's order per image: [mocov3: the RandomResizedCrop box, needs `sizes` =
        [(h, w)] of the images], flip (torch.rand(1) < 0.5), angle (uniform in [-rotate, rotate]), crop offsets (randint);
        evaluation: no flip, no rotation, CenterCrop offsets.  Tuples (flip, angle, crop_i, crop_j[, box]).  maintain_ratio
        needs `sizes` too: the offsets range over each image's own frame, and RandomCrop draws nothing when the frame equals the
        crop."""
        S, C = self.size, self.crop
        if (self.maintain_ratio or (self.training and self.mocov3)) and (sizes is None or len(sizes) < n):
            raise _lib.MfvitError("sample_params needs the (h, w) of every image (sizes)")
        out = []
        for s in range(n):
            if self.training and self.mocov3:
                box = self.resized_crop_box(sizes[s][0], sizes[s][1], (self.crop_min, 1.0), generator)
                flip = bool(torch.rand(1, generator=generator) < 0.5)
                angle = float(torch.empty(1).uniform_(-self.rotate, self.rotate, generator=generator))
                out.append((flip, angle, 0, 0, box))
                continue
            if self.maintain_ratio:
                out.append(self._ratio_params(*self.frame(*sizes[s][:2]), generator))
                continue
            if self.training:
                flip = bool(torch.rand(1, generator=generator) < 0.5)
                angle = float(torch.empty(1).uniform_(-self.rotate, self.rotate, generator=generator))
                i = int(torch.randint(0, S - C + 1, (1,), generator=generator))
                j = int(torch.randint(0, S - C + 1, (1,), generator=generator))
            else:
                flip, angle = False, 0.0
                i = j = int(round((S - C) / 2.0))
            out.append((flip, angle, i, j))
        return out

    def _ratio_params(self, fh, fw, generator):
        """(flip, angle, i, j) of one fh x fw frame: RandomCrop.get_params / CenterCrop offsets (no crop: (0, 0), nothing drawn)."""
        C = self.crop
        if not self.no_crop and (fh < C or fw < C):
            raise _lib.MfvitError(f"crop {C} larger than the resized frame {fh} x {fw}")
        if not self.training:
            if self.no_crop:
                return False, 0.0, 0, 0
            return False, 0.0, int(round((fh - C) / 2.0)), int(round((fw - C) / 2.0))
        flip = bool(torch.rand(1, generator=generator) < 0.5)
        angle = float(torch.empty(1).uniform_(-self.rotate, self.rotate, generator=generator))
        if self.no_crop or (fh == C and fw == C):
            return flip, angle, 0, 0
        i = int(torch.randint(0, fh - C + 1, (1,), generator=generator))
        j = int(torch.randint(0, fw - C + 1, (1,), generator=generator))
        return flip, angle, i, j

    def sample_view_pairs(self, n, generator=None, sizes=None):
        """[(q_params, k_params)] of two_views: all of image 0's q draws, then its k draws, then image 1's, ... - the order of
        Dataset_covid.__getitem__ inside one DataLoader worker."""
        sizes = [None] * n if sizes is None else sizes
        return [tuple(self.sample_params(1, generator, None if sz is None else [sz])[0] for _ in range(2)) for sz in sizes[:n]]

    @staticmethod
    def _arrays(images):
        arrs = []
        for im in images:
            a = im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise _lib.MfvitError("images must be uint8 HWC with 3 channels (Image.fromarray(cv2.imread(..)), loader.py:121-125)")
            arrs.append(np.ascontiguousarray(a))
        return arrs

    def __call__(self, images, params=None, generator=None):
        """images: list of uint8 HWC (3-channel) numpy arrays / CPU tensors of any size.  Returns float32 [n, 3, crop, crop] on
        the device ([n, 3, Sh, Sw] for maintain_ratio without a crop, when every frame is Sh x Sw).  params: list of
        (flip, angle, crop_i, crop_j) per image (default: sample_params)."""
        arrs = self._arrays(images)
        if params is None:
            params = self.sample_params(len(arrs), generator, [a.shape[:2] for a in arrs])
        if len(params) != len(arrs):
            raise _lib.MfvitError(f"{len(params)} params for {len(arrs)} images")
        return self._run(arrs, list(enumerate(params)))

    def two_views(self, images, params=None, generator=None):
        """MoCo's two views (Dataset_covid.__getitem__, moco/loader.py:121-137: the random transform applied twice to one decoded
        image): (q, k), each float32 [n, 3, crop, crop].  Every source is uploaded once and all 2n samples run in one launch.
        params: list of (q_params, k_params) pairs (default: sample_view_pairs)."""
        arrs = self._arrays(images)
        n = len(arrs)
        if params is None:
            params = self.sample_view_pairs(n, generator, [a.shape[:2] for a in arrs])
        if len(params) != n or not all(isinstance(p, (tuple, list)) and len(p) == 2 and
                                        all(isinstance(v, (tuple, list)) and len(v) in (4, 5) for v in p) for p in params):
            raise _lib.MfvitError("two_views params: one (q_params, k_params) pair per image, each (flip, angle, crop_i, crop_j[, box])")
        out = self._run(arrs, [(s, p[0]) for s, p in enumerate(params)] + [(s, p[1]) for s, p in enumerate(params)])
        return out[:n], out[n:]

    def _run(self, arrs, samples):
        """One launch over `samples` = [(source index, params)]; each source is uploaded once."""
        n = len(samples)
        S, C = self.size, self.crop
        offs, off = [], 0
        for a in arrs:
            offs.append(off)
            off += a.size
        desc = np.zeros((n, 20), dtype=np.int64)
        tabs, tab_off, tab_pos = [], {}, 0
        out_hw = None
        for s, (src_i, prm) in enumerate(samples):
            a = arrs[src_i]
            flip, angle, ci, cj = prm[:4]
            H, W = a.shape[:2]
            bi, bj, h, w = prm[4] if len(prm) > 4 else (0, 0, H, W)      # source window (RandomResizedCrop box) or the whole image
            if not (0 <= bi and 0 <= bj and h > 0 and w > 0 and bi + h <= H and bj + w <= W):
                raise _lib.MfvitError("source window outside the image")
            fh, fw = self.frame(h, w)
            oh, ow = (fh, fw) if self.maintain_ratio and self.no_crop else (C, C)
            if out_hw is None:
                out_hw = (oh, ow)
            elif out_hw != (oh, ow):
                raise _lib.MfvitError(f"maintain_ratio without a crop: resized frames {out_hw} and {(oh, ow)} cannot form one batch")
            for key in ((w, fw), (h, fh)):
                if key not in tab_off:
                    ks, t = axis_table(*key)
                    tab_off[key] = (tab_pos, ks)
                    tabs.append(t.reshape(-1))
                    tab_pos += t.size
            mode, terms = rotation_terms(angle, fw, fh)
            if not (0 <= ci <= fh - oh and 0 <= cj <= fw - ow):
                raise _lib.MfvitError("crop offset out of range")
            tx, ty = tab_off[(w, fw)], tab_off[(h, fh)]
            desc[s] = [offs[src_i] + (bi * W + bj) * 3, h, w, tx[0], ty[0], tx[1], ty[1], int(flip), mode, *terms, (ci << 32) | cj, W * 3,
                       (fh << 32) | fw if self.maintain_ratio else 0, 0, 0]
        if not torch.cuda.is_available():
            raise _lib.MfvitError("GpuTransform needs the GPU (no CPU fallback)")
        src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(self.device, non_blocking=True)
        dsc = torch.from_numpy(desc).to(self.device, non_blocking=True)
        tab = torch.from_numpy(np.concatenate(tabs)).to(self.device, non_blocking=True)
        out = torch.empty(n, 3, *out_hw, device=self.device, dtype=torch.float32)
        mean = (ctypes.c_float * 3)(*self.mean)
        std = (ctypes.c_float * 3)(*self.std)
        check(lib().mfvit_input_transform_rect(ptr(src), ptr(dsc), ptr(tab), n, S, out_hw[0], out_hw[1], ctypes.cast(mean, ctypes.c_void_p),
                                               ctypes.cast(std, ctypes.c_void_p), ptr(out), stream()), "mfvit_input_transform_rect")
        return out
