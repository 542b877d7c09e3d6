"""TEST INFRASTRUCTURE ONLY: numpy restatement of the photometric half of the MoCo-v3 aug1 / aug2 chains
(main_covid_mocov3based_..._vitsmall.py:388-413) - ColorJitter, RandomGrayscale, moco.loader.GaussianBlur, Solarize - as torchvision's
PIL backend computes them: ImageEnhance (ImagingBlend), Image.convert (L, HSV), ImageFilter.GaussianBlur (three extended box blurs per
axis) and ImageOps.solarize, in Pillow's integers, float32 and doubles.  tests/test_photometric_cpu.py pins every function against the
installed Pillow, bit for bit; the whole chain sits on top of oracle.ref_input's resize.

The MUTATIONS are deliberate errors (a blend in double, an all-float32 hue, a double box weight, an edge clamp at the tile edge): the CPU
test shows that the inputs of the GPU test catch each of them."""
import numpy as np

from oracle import ref_input

F32 = np.float32
MUTATIONS = ("blend_double", "hue_f32", "ww_double", "tile_clamp")
TILE = 32                                  # the blur tile of csrc/photometric.hip (the tile_clamp mutation clamps at its edges)
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3        # torchvision ColorJitter's fn_idx


def luma(img):
    """Image.convert('L') of uint8 HWC RGB: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    x = img.astype(np.int64)
    return ((19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f, mutation=None):
    """ImagingBlend(deg, img, f) = ImageEnhance's deg + f (img - deg), in float32 (mutation blend_double: in double)."""
    ft = np.float64 if mutation == "blend_double" else F32
    f = ft(F32(f))
    t = deg.astype(ft) + f * (img.astype(np.int32) - deg.astype(np.int32)).astype(ft)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def brightness(img, f, mutation=None):
    return blend(np.zeros_like(img), img, f, mutation)


def saturation(img, f, mutation=None):
    return blend(np.repeat(luma(img)[..., None], 3, axis=2), img, f, mutation)


def contrast_mean(img):
    """int(mean(L) + 0.5) from the exact integer sum."""
    total, count = int(luma(img).astype(np.int64).sum()), img.shape[0] * img.shape[1]
    return (2 * total + count) // (2 * count)


def contrast(img, f, mutation=None):
    return blend(np.full_like(img, contrast_mean(img)), img, f, mutation)


def rgb2hsv(img, mutation=None):
    """Pillow's rgb2hsv_row: float32, with the g / b hue branches, the fmod and the two scalings in double."""
    x = img.astype(np.int32)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    mx, mn = x.max(axis=-1), x.min(axis=-1)
    gray = mx == mn
    dt = F32 if mutation == "hue_f32" else np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(F32)
        s = cr / mx.astype(F32)
        rc, gc, bc = ((mx - c).astype(F32) / cr for c in (r, g, b))
        h_r = bc - gc
        h_g = ((dt(2.0) + rc.astype(dt)) - bc.astype(dt)).astype(F32)
        h_b = ((dt(4.0) + gc.astype(dt)) - rc.astype(dt)).astype(F32)
        h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
        h = np.fmod(h.astype(dt) / dt(6.0) + dt(1.0), dt(1.0)).astype(F32)
        uh = np.clip((h.astype(dt) * dt(255.0)).astype(np.int64), 0, 255)
        us = np.clip((s.astype(dt) * dt(255.0)).astype(np.int64), 0, 255)
    uh, us = np.where(gray, 0, uh), np.where(gray, 0, us)
    return np.stack([uh, us, mx], axis=-1).astype(np.uint8)


def _round_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv2rgb(hsv):
    """Pillow's hsv2rgb: fs, h6 float32; p, q, t from double products rounded to float, then half away from zero, clipped."""
    h, s, v = (hsv[..., k].astype(np.float64) for k in range(3))
    fs = (s / 255.0).astype(F32)
    h6 = (h * 6.0 / 255.0).astype(F32)
    i = np.floor(h6)
    f = (h6 - i).astype(np.float64)
    fs = fs.astype(np.float64)
    rnd = lambda a: np.clip(_round_away((v * a).astype(F32).astype(np.float64)), 0, 255).astype(np.uint8)
    p, q, t = rnd(1.0 - fs), rnd(1.0 - fs * f), rnd(1.0 - fs * (1.0 - f))
    vv = hsv[..., 2]
    sel = i.astype(np.int64) % 6
    r = np.choose(sel, [vv, q, p, p, t, vv])
    g = np.choose(sel, [t, vv, vv, q, p, p])
    b = np.choose(sel, [p, p, t, vv, vv, q])
    out = np.stack([r, g, b], axis=-1)
    return np.where((hsv[..., 1] == 0)[..., None], vv[..., None], out).astype(np.uint8)


def hue_shift(hue):
    """torchvision adjust_hue: np.int32(hue * 255) (truncated toward zero) wrapped to uint8."""
    return int(float(hue) * 255) & 255


def hue(img, hue_factor, mutation=None):
    hsv = rgb2hsv(img, mutation)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(hue_factor)) & 255
    return hsv2rgb(hsv)


def grayscale(img):
    return np.repeat(luma(img)[..., None], 3, axis=2)


def solarize(img):
    return np.where(img < 128, img, 255 - img).astype(np.uint8)


def box_params(sigma, mutation=None):
    """(r, ww, fw) of one pass of ImageFilter.GaussianBlur(sigma): _gaussian_blur_radius and ImagingLineBoxBlur8's weights, float32
    throughout (mutation ww_double: the weight's division in double)."""
    sigma = F32(sigma)
    sigma2 = sigma * sigma / F32(3)
    L = np.sqrt(F32(12) * sigma2 + F32(1))
    l = np.floor((L - F32(1)) / F32(2))
    a = (F32(2) * l + F32(1)) * (l * (l + F32(1)) - F32(3) * sigma2)
    a = a / (F32(6) * (sigma2 - (l + F32(1)) * (l + F32(1))))
    fr = F32(l + a)
    r = int(fr)
    if mutation == "ww_double":
        ww = int(float(1 << 24) / (float(fr) * 2 + 1))
    else:
        ww = int(F32(1 << 24) / (fr * F32(2) + F32(1)))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def _box_pass(x, r, ww, fw, axis, lo=None, hi=None):
    """One extended box pass along `axis` of an int64 HWC array; indices clamp to [lo, hi] (default: the image edge)."""
    n = x.shape[axis]
    idx = np.arange(n)
    lo = np.zeros(n, dtype=np.int64) if lo is None else lo
    hi = np.full(n, n - 1, dtype=np.int64) if hi is None else hi
    take = lambda d: np.take(x, np.clip(idx + d, lo, hi), axis=axis)
    acc = sum(take(d) for d in range(-r, r + 1))
    return (ww * acc + fw * (take(-r - 1) + take(r + 1)) + (1 << 23)) >> 24


def gaussian_blur(img, sigma, mutation=None):
    """ImageFilter.GaussianBlur(radius=sigma): three passes along rows, then three along columns, each on the uint8 result of the last."""
    r, ww, fw = box_params(sigma, mutation)
    x = img.astype(np.int64)
    for axis in (1, 0):
        lo = hi = None
        if mutation == "tile_clamp":
            idx = np.arange(x.shape[axis])
            lo, hi = idx // TILE * TILE, np.minimum(idx // TILE * TILE + TILE - 1, x.shape[axis] - 1)
        for _ in range(3):
            x = _box_pass(x, r, ww, fw, axis, lo, hi)
    return x.astype(np.uint8)


def photometric(img, photo, mutation=None):
    """The photometric operations of one sample on a uint8 HWC frame.  photo = (order, b, c, s, h, gray, sigma, solarize): order the
    tuple of ColorJitter's fn_idx or None (jitter off), sigma None = blur off."""
    order, fb, fc, fs, fh, gray, sigma, sol = photo
    for op in order or ():
        if op == BRIGHTNESS:
            img = brightness(img, fb, mutation)
        elif op == CONTRAST:
            img = contrast(img, fc, mutation)
        elif op == SATURATION:
            img = saturation(img, fs, mutation)
        else:
            img = hue(img, fh, mutation)
    if gray:
        img = grayscale(img)
    if sigma is not None:
        img = gaussian_blur(img, sigma, mutation)
    if sol:
        img = solarize(img)
    return img


def transform_photo(img, box, size, flip, photo, mean, std, mutation=None):
    """aug1 / aug2 for ONE decoded uint8 HWC image with the draws given: RandomResizedCrop box -> resize (oracle.ref_input) -> jitter ->
    grayscale -> blur -> solarize -> flip (last, as the reference) -> ToTensor -> Normalize."""
    i, j, h, w = box
    x = ref_input.resize_bilinear_u8(ref_input.crop(img, i, j, h, w), size, size)
    x = photometric(x, photo, mutation)
    if flip:
        x = ref_input.hflip(x)
    return ref_input.to_tensor_normalize(x, mean, std)


# ---- the inputs of tests/test_photometric_gpu.py (shared with the mutation check of tests/test_photometric_cpu.py)
import functools
import itertools

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SOURCES = ((40, 56), (33, 47), (64, 64), (9, 70))
SIZES = (32, 40, 45)                               # one tile; two tiles per axis; 45 is no multiple of the tile, odd
SENSITIVE_SIGMAS = (0.3, 1.0, 1.2247449, 1.7320508)
FACTORS = (0.6, 0.83, 1.0, 1.17, 1.4)
HUES = (-0.5, -0.1, -0.03, 0.0, 0.07, 0.1, 0.5)
SIGMAS = (None, 0.1) + SENSITIVE_SIGMAS + (2.0, 1.4142134, 1.42)      # blur off, r = 0 (up to 1.4142134), r = 1


@functools.lru_cache(maxsize=None)
def images():
    """Decoded sources: random pixels, and one smooth image (64 x 64) where neighbouring hues and the blur's rounding are close calls."""
    rng = np.random.Generator(np.random.PCG64(21))
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SOURCES]
    y, x = np.mgrid[0:64, 0:64]
    smooth = np.stack([2 * x + y, 255 - 3 * y, x + 2 * y + 40], axis=-1) + rng.integers(0, 3, (64, 64, 3))
    imgs[2] = np.clip(smooth, 0, 255).astype(np.uint8)
    return imgs


def boxes(h, w):
    """RandomResizedCrop windows: the whole image, the two corners (each touches the border), an interior window."""
    return ((0, 0, h, w), (0, 0, max(h // 2, 1), w // 2), (h - max(h // 3, 1), w - w // 3, max(h // 3, 1), w // 3), (1, 3, h - 3, w - 7))


def samples():
    """[(source index, flip, box, photo)]: the 24 jitter orders, then jitter off / single factors / every sigma - factors on both sides
    of 1 and exactly 1, hue shifts of both signs that wrap, gray, blur (off, r = 0, r = 1, the rounding-sensitive sigmas), solarize
    and flip on and off, boxes on the border; every sample of the list differs from its neighbours in the descriptor."""
    out = []
    for k, order in enumerate(itertools.permutations(range(4))):
        src = k % 4
        photo = (order, FACTORS[k % 5], FACTORS[(k + 1) % 5], FACTORS[(k + 3) % 5], HUES[k % 7], k % 3 == 0, SIGMAS[k % 9], k % 4 == 1)
        out.append((src, k % 2 == 1, boxes(*SOURCES[src])[(k // 4) % 4], photo))
    for k, sigma in enumerate(SIGMAS):                                                  # jitter off
        src = (k + 1) % 4
        out.append((src, k % 2 == 0, boxes(*SOURCES[src])[k % 4], (None, None, None, None, None, k % 2 == 1, sigma, k % 3 == 0)))
    for k, f in enumerate(FACTORS):                                                     # contrast first / last, and alone
        out.append((2, False, boxes(64, 64)[0], ((1, 0, 2, 3), f, f, f, HUES[k], False, None, False)))
        out.append((0, True, boxes(40, 56)[3], ((3, 2, 0, 1), 1.0, f, 1.0, 0.0, False, SIGMAS[k + 2], True)))
    return out


@functools.lru_cache(maxsize=None)
def reference(size, mutation=None):
    """The restatement's float32 [n, 3, size, size] for samples() (computed once per size)."""
    imgs = images()
    return np.stack([transform_photo(imgs[src], box, size, flip, photo, MEAN, STD, mutation) for src, flip, box, photo in samples()])
