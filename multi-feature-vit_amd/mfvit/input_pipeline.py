"""GPU-side input pipeline: the finetune transform chain of aihc_utils/image_transform.py:50-84 as one HIP kernel.

    tf = GpuTransform(img_type="CheXpert-v1.0-small", img_size=256, crop=224, rotate=10, training=True, maintain_ratio=True)
    batch = tf(list_of_uint8_HWC_arrays)            # float32 [B, 3, 224, 224] on the GPU, what the DataLoader used to deliver
    q, k = tf.two_views(list_of_uint8_HWC_arrays)   # MoCo: two random views of each image (moco/loader.py:121-137)

The DataLoader workers then only decode (cv2.imread, moco/loader.py:121) and hand over uint8 HWC arrays of any size; Resize((S,S))
or Resize(S) (maintain_ratio: shorter side S) -> RandomHorizontalFlip -> RandomRotation(rotate) -> RandomCrop((crop,crop)) |
CenterCrop -> ToTensor -> Normalize run fused on the device, bit-exact against Pillow's integer arithmetic (the backend
torchvision's PIL transforms call).  This module is the host half: the per-axis fixed-point coefficient tables and the 16.16
affine terms, computed in double exactly as Pillow does.

    tf = GpuTransform("imagenet", img_size=224, mocov3=True, photometric=(AUG1, AUG2))
    q, k = tf.two_views(list_of_uint8_HWC_arrays)   # MoCo-v3's TwoCropsTransform(aug1, aug2) with the colour operations on the device

`Photometric` adds the colour half of the MoCo pretraining driver's `aug1` / `aug2` settings
(main_covid_mocov3based_..._vitsmall.py:388-413): ColorJitter, RandomGrayscale, GaussianBlur and Solarize, bit-exact against Pillow.
"""
import collections
import ctypes
import dataclasses
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
    "imagenet": ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]),       # the MoCo driver's own Normalize (main_covid_mocov3based_...:385-386)
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


# The photometric draws of one sample.  order: ColorJitter's fn_idx permutation (0 brightness, 1 contrast, 2 saturation, 3 hue) or None
# when RandomApply skipped the jitter; brightness / contrast / saturation the enhance factors, hue the shift in [-0.5, 0.5] (None: that
# operation is not part of the recipe); gray, solarize bools; sigma the blur radius or None (no blur).
PhotoParams = collections.namedtuple("PhotoParams", "order brightness contrast saturation hue gray sigma solarize")
MAX_BOX_RADIUS = 1          # csrc/photometric.hip's blur tile: r <= 1, which is sigma <= 2.4494896


def box_blur_terms(sigma):
    """(r, ww, fw) of one pass of ImageFilter.GaussianBlur(radius=sigma): libImaging's _gaussian_blur_radius(sigma, 3) and the
    weights of ImagingLineBoxBlur8, in float32 throughout as the C code has them (a double anywhere changes ww at some sigmas)."""
    f = np.float32
    sigma2 = f(sigma) * f(sigma) / f(3)
    L = np.sqrt(f(12) * sigma2 + f(1))
    l = np.floor((L - f(1)) / f(2))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2)
    a = a / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    fr = f(l + a)
    r = int(fr)
    ww = int(f(1 << 24) / (fr * f(2) + f(1)))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


@dataclasses.dataclass(frozen=True)
class Photometric:
    """One recipe of the colour operations between RandomResizedCrop and the flip (main_covid_mocov3based_..._vitsmall.py:388-413):
    RandomApply([ColorJitter(brightness, contrast, saturation, hue)], p=jitter_p) -> RandomGrayscale(gray_p) ->
    RandomApply([GaussianBlur(sigma)], p=blur_p) -> RandomApply([Solarize()], p=solarize_p) (left out of the chain at 0).

    Deviations from the reference: sigma comes from the torch generator (moco/loader.py:32 draws it from Python's global `random`);
    `moco.loader.Solarize` is missing from the reference's loader.py, so this is upstream MoCo-v3's, ImageOps.solarize at threshold 128."""
    jitter_p: float = 0.8
    brightness: float = 0.4
    contrast: float = 0.4
    saturation: float = 0.2
    hue: float = 0.1
    gray_p: float = 0.2
    blur_p: float = 1.0
    sigma: tuple = (0.1, 2.0)
    solarize_p: float = 0.0

    def sample(self, generator=None):
        """The draws of one sample, in the order torchvision's transforms make them (restated from its source; torchvision is not
        a dependency): RandomApply's torch.rand(1) (the jitter applies if p >= rand); if it applies torch.randperm(4), then the
        brightness, contrast, saturation factors from [max(0, 1 - x), 1 + x] and the hue from [-hue, hue], each by
        torch.empty(1).uniform_; RandomGrayscale's rand < p; the blur's RandomApply rand (drawn even at p = 1); sigma if the blur
        applies; the solarize rand if the recipe has one."""
        uni = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=generator))
        skip = lambda p: bool(p < torch.rand(1, generator=generator))           # RandomApply.forward
        order = b = c = sa = h = None
        if not skip(self.jitter_p):
            order = tuple(int(v) for v in torch.randperm(4, generator=generator))
            b, c, sa = (uni(max(0.0, 1.0 - x), 1.0 + x) if x else None for x in (self.brightness, self.contrast, self.saturation))
            h = uni(-self.hue, self.hue) if self.hue else None
        gray = bool(torch.rand(1, generator=generator) < self.gray_p)
        sigma = None if skip(self.blur_p) else uni(self.sigma[0], self.sigma[1])
        solarize = bool(self.solarize_p) and not skip(self.solarize_p)
        return PhotoParams(order, b, c, sa, h, gray, sigma, solarize)


# the reference's numbers (main_covid_mocov3based_..._vitsmall.py:390-413)
AUG1 = Photometric()
AUG2 = Photometric(blur_p=0.1, solarize_p=0.2)


def photo_descriptor(photo):
    """(int32 [16] descriptor of include/mfvit.h's mfvit_input_photometric, box radius) of one sample's PhotoParams."""
    order, b, c, sa, h, gray, sigma, solarize = photo
    bits = lambda v: int(np.float32(1.0 if v is None else v).view(np.int32))
    d = np.zeros(16, dtype=np.int32)
    factors = (b, c, sa, h)
    if order is not None:
        if sorted(order) != [0, 1, 2, 3]:
            raise _lib.MfvitError("photo order: a permutation of (0, 1, 2, 3) or None")
        ops = [op + 1 for op in order if factors[op] is not None]
        d[0] = sum(code << (4 * k) for k, code in enumerate(ops))
    d[1], d[2], d[3] = bits(b), bits(c), bits(sa)
    if h is not None:
        if not -0.5 <= h <= 0.5:
            raise _lib.MfvitError("hue shift outside [-0.5, 0.5]")
        d[4] = int(float(h) * 255) & 255                   # torchvision adjust_hue: np.int32(hue * 255) wrapped to uint8
    r = 0
    if sigma is not None:
        r, ww, fw = box_blur_terms(sigma)
        d[6], d[7], d[8] = r, ww, fw
    d[5] = int(bool(gray)) | (int(sigma is not None) << 1) | (int(bool(solarize)) << 2)
    return d, r


class GpuTransform:
    """Mirror of `get_transform_type(args, training, img_type)` (image_transform.py:50-84): args.img_size -> img_size, args.crop ->
    crop (0 = no crop), args.rotate -> rotate (degrees; RandomRotation draws from [-rotate, rotate]), args.maintain_ratio ->
    maintain_ratio (False: Resize((S, S)) squashes every image to a square; True: Resize(S), the shorter side becomes S and the
    aspect ratio is kept)."""

    def __init__(self, img_type="CheXpert-v1.0-small", img_size=256, crop=224, rotate=10, training=True, device="cuda:0",
                 mocov3=False, crop_min=0.08, maintain_ratio=False, photometric=None):
        """mocov3=True mirrors `get_transform_type_mocov3` (image_transform.py:86-124, MoCo pretraining): training =
        RandomResizedCrop(img_size, scale=(crop_min, 1)) -> flip -> rotation (no further crop; maintain_ratio has no effect);
        evaluation = Resize((256, 256)) | Resize(256) (maintain_ratio) -> CenterCrop(crop).
        photometric (with mocov3=True, training): a `Photometric` recipe, or a pair (q recipe, k recipe) for `two_views` (upstream
        MoCo-v3's TwoCropsTransform(aug1, aug2)), selects the driver's aug1 / aug2 chains: RandomResizedCrop -> the recipe's colour
        operations -> flip; no rotation and no crop after the resize."""
        self.mocov3, self.crop_min = bool(mocov3), float(crop_min)
        if photometric is not None:
            if not (mocov3 and training):
                raise _lib.MfvitError("photometric recipes belong to the MoCo training chain (mocov3=True, training=True)")
            photometric = (photometric, photometric) if isinstance(photometric, Photometric) else tuple(photometric)
            if len(photometric) != 2 or not all(isinstance(r, Photometric) for r in photometric):
                raise _lib.MfvitError("photometric: one Photometric or a (q, k) pair of them")
        self.photometric = photometric
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

    def sample_params(self, n, generator=None, sizes=None, recipe=None):
        """The random draws of one batch, in torchvision's order per image: [mocov3: the RandomResizedCrop box, needs `sizes` =
        [(h, w)] of the images], flip (torch.rand(1) < 0.5), angle (uniform in [-rotate, rotate]), crop offsets (randint);
        evaluation: no flip, no rotation, CenterCrop offsets.  Tuples (flip, angle, crop_i, crop_j[, box]).  maintain_ratio
        needs `sizes` too: the offsets range over each image's own frame, and RandomCrop draws nothing when the frame equals the
        crop.  With a photometric recipe (`recipe`, default the q recipe) a sample draws the box, then `Photometric.sample`'s draws,
        then the flip - the order of the aug1 / aug2 transform lists - and the tuple is (flip, 0.0, 0, 0, box, PhotoParams)."""
        S, C = self.size, self.crop
        if (self.maintain_ratio or (self.training and self.mocov3)) and (sizes is None or len(sizes) < n):
            raise _lib.MfvitError("sample_params needs the (h, w) of every image (sizes)")
        out = []
        for s in range(n):
            if self.training and self.mocov3:
                box = self.resized_crop_box(sizes[s][0], sizes[s][1], (self.crop_min, 1.0), generator)
                if self.photometric:
                    photo = (recipe or self.photometric[0]).sample(generator)
                    out.append((bool(torch.rand(1, generator=generator) < 0.5), 0.0, 0, 0, box, photo))
                    continue
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
        Dataset_covid.__getitem__ inside one DataLoader worker.  With photometric recipes q draws from the first, k from the second."""
        sizes = [None] * n if sizes is None else sizes
        recipes = self.photometric or (None, None)
        return [tuple(self.sample_params(1, generator, None if sz is None else [sz], r)[0] for r in recipes) for sz in sizes[:n]]

    @staticmethod
    def _with_photo(prm, photo):
        return tuple(prm[:4]) + (prm[4] if len(prm) > 4 else None, PhotoParams(*photo))

    @staticmethod
    def _arrays(images):
        arrs = []
        for im in images:
            a = im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise _lib.MfvitError("images must be uint8 HWC with 3 channels (Image.fromarray(cv2.imread(..)), loader.py:121-125)")
            arrs.append(np.ascontiguousarray(a))
        return arrs

    def __call__(self, images, params=None, generator=None, photo=None):
        """images: list of uint8 HWC (3-channel) numpy arrays / CPU tensors of any size.  Returns float32 [n, 3, crop, crop] on
        the device ([n, 3, Sh, Sw] for maintain_ratio without a crop, when every frame is Sh x Sw).  params: list of
        (flip, angle, crop_i, crop_j) per image (default: sample_params).  photo (photometric chains): one PhotoParams (or plain
        8-tuple) per image, replacing the drawn ones."""
        arrs = self._arrays(images)
        if params is None:
            params = self.sample_params(len(arrs), generator, [a.shape[:2] for a in arrs])
        if len(params) != len(arrs):
            raise _lib.MfvitError(f"{len(params)} params for {len(arrs)} images")
        if photo is not None:
            if len(photo) != len(arrs):
                raise _lib.MfvitError(f"{len(photo)} photo entries for {len(arrs)} images")
            params = [self._with_photo(p, ph) for p, ph in zip(params, photo)]
        return self._run(arrs, list(enumerate(params)))

    def two_views(self, images, params=None, generator=None, photo=None):
        """MoCo's two views (Dataset_covid.__getitem__, moco/loader.py:121-137: the random transform applied twice to one decoded
        image): (q, k), each float32 [n, 3, crop, crop].  Every source is uploaded once and all 2n samples run in one launch.
        params: list of (q_params, k_params) pairs (default: sample_view_pairs).  photo (photometric chains): one
        (q PhotoParams, k PhotoParams) pair per image, replacing the drawn ones."""
        arrs = self._arrays(images)
        n = len(arrs)
        if params is None:
            params = self.sample_view_pairs(n, generator, [a.shape[:2] for a in arrs])
        if len(params) != n or not all(isinstance(p, (tuple, list)) and len(p) == 2 and
                                        all(isinstance(v, (tuple, list)) and len(v) in (4, 5, 6) for v in p) for p in params):
            raise _lib.MfvitError("two_views params: one (q_params, k_params) pair per image, each (flip, angle, crop_i, crop_j[, box])")
        if photo is not None:
            if len(photo) != n or not all(len(ph) == 2 for ph in photo):
                raise _lib.MfvitError("two_views photo: one (q, k) pair of PhotoParams per image")
            params = [tuple(self._with_photo(v, f) for v, f in zip(p, ph)) for p, ph in zip(params, photo)]
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
        pdesc, max_r = np.zeros((n, 16), dtype=np.int32), 0
        tabs, tab_off, tab_pos = [], {}, 0
        out_hw = None
        for s, (src_i, prm) in enumerate(samples):
            a = arrs[src_i]
            flip, angle, ci, cj = prm[:4]
            H, W = a.shape[:2]
            bi, bj, h, w = prm[4] if len(prm) > 4 and prm[4] is not None else (0, 0, H, W)      # source window (RandomResizedCrop box) or the whole image
            if self.photometric:
                if len(prm) < 6 or angle or ci or cj:
                    raise _lib.MfvitError("a photometric chain takes (flip, 0.0, 0, 0, box, PhotoParams): no rotation, no crop")
                pdesc[s], r = photo_descriptor(prm[5])
                max_r = max(max_r, r)
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
        if self.photometric:
            pds = torch.from_numpy(pdesc).to(self.device, non_blocking=True)
            ws = torch.empty(lib().mfvit_input_photometric_workspace_bytes(n, S), device=self.device, dtype=torch.uint8)
            check(lib().mfvit_input_photometric(ptr(src), ptr(dsc), ptr(tab), ptr(pds), n, S, max_r, ptr(ws), ctypes.cast(mean, ctypes.c_void_p),
                                                ctypes.cast(std, ctypes.c_void_p), ptr(out), stream()), "mfvit_input_photometric")
            return out
        check(lib().mfvit_input_transform_rect(ptr(src), ptr(dsc), ptr(tab), n, S, out_hw[0], out_hw[1], ctypes.cast(mean, ctypes.c_void_p),
                                               ctypes.cast(std, ctypes.c_void_p), ptr(out), stream()), "mfvit_input_transform_rect")
        return out
