"""CPU: the restatement of the MoCo-v3 aug1 / aug2 colour operations (tests/photometric_ref.py) and the host half of
mfvit.input_pipeline.Photometric.
  - every operation of the restatement equals the installed Pillow (what torchvision's PIL backend calls), bit for bit;
  - whole chains in all 24 jitter orders equal the same calls made on a PIL.Image in the same order;
  - the draws come in the written order (Photometric.sample's docstring), and a chain without a recipe draws what it always drew;
  - the restatement with a blend in double, an all-float32 hue, a double box weight or a clamp at the tile edge is caught by the inputs
    of tests/test_photometric_gpu.py;
  - the host's box-blur terms and descriptors, the presets and the C ABI declarations."""
import itertools
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

import photometric_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (0.6, 0.83, 1.0, 1.17, 1.4)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _images():
    """A random and a smooth 37 x 53 RGB image."""
    y, x = np.mgrid[0:37, 0:53]
    smooth = np.stack([3 * x + y, 250 - 4 * y, 2 * x + 3 * y], axis=-1) + _rng(2).integers(0, 3, (37, 53, 3))
    return [_rng(1).integers(0, 256, (37, 53, 3), dtype=np.uint8), np.clip(smooth, 0, 255).astype(np.uint8)]


def pil_hue(pim, hue):
    """torchvision's adjust_hue on a PIL image (functional_pil.py), restated: H += np.int32(hue * 255) as uint8, in Pillow's HSV."""
    h, s, v = pim.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h = (np_h.astype(np.int32) + int(np.int32(hue * 255).astype(np.uint8))).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


PIL_OPS = {ref.BRIGHTNESS: lambda im, f: ImageEnhance.Brightness(im).enhance(f), ref.CONTRAST: lambda im, f: ImageEnhance.Contrast(im).enhance(f),
           ref.SATURATION: lambda im, f: ImageEnhance.Color(im).enhance(f), ref.HUE: pil_hue}


@pytest.mark.parametrize("f", FACTORS)
def test_enhance_equals_pillow(f):
    for img in _images():
        pim = Image.fromarray(img)
        assert np.array_equal(ref.luma(img), np.asarray(pim.convert("L")))
        assert np.array_equal(ref.brightness(img, f), np.asarray(PIL_OPS[ref.BRIGHTNESS](pim, f)))
        assert np.array_equal(ref.contrast(img, f), np.asarray(PIL_OPS[ref.CONTRAST](pim, f)))
        assert np.array_equal(ref.saturation(img, f), np.asarray(PIL_OPS[ref.SATURATION](pim, f)))


def test_contrast_mean_rounds_as_pillow():
    """Constant images, and images whose L mean sits just below and just above x.5 (one pixel of 1000 decides)."""
    for v in (0, 1, 127, 128, 255):
        img = np.full((5, 7, 3), v, dtype=np.uint8)
        assert ref.contrast_mean(img) == v
        assert np.array_equal(ref.contrast(img, 1.4), np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(1.4)))
    for ones, want in ((499, 100), (500, 101), (501, 101)):          # mean L = 100.499, 100.5, 100.501
        img = np.full((25, 40, 3), 100, dtype=np.uint8)
        img.reshape(-1, 3)[:ones] = 101
        assert ref.contrast_mean(img) == want
        for f in (0.6, 1.4):
            assert np.array_equal(ref.contrast(img, f), np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f)))


def _hsv_pixels():
    g = np.arange(256, dtype=np.uint8)
    gray = np.stack([g, g, g], axis=-1)
    sat = np.array([p for p in itertools.product((0, 1, 127, 128, 254, 255), repeat=3)], dtype=np.uint8)
    return np.concatenate([gray, sat, _rng(3).integers(0, 256, (20000, 3), dtype=np.uint8)])[None]


def test_hsv_both_ways_equals_pillow():
    px = _hsv_pixels()
    assert np.array_equal(ref.rgb2hsv(px), np.asarray(Image.fromarray(px, "RGB").convert("HSV")))
    assert np.array_equal(ref.hsv2rgb(px), np.asarray(Image.fromarray(px, "HSV").convert("RGB")))       # the same bytes read as H, S, V
    assert not np.array_equal(ref.rgb2hsv(px, "hue_f32"), ref.rgb2hsv(px))


@pytest.mark.parametrize("hue", [-0.5, -0.3, -0.1, -0.004, 0.0, 0.003, 0.1, 0.25, 0.5])
def test_hue_shift_equals_pillow(hue):
    assert ref.hue_shift(hue) == int(np.int32(hue * 255).astype(np.uint8))
    for img in _images() + [_hsv_pixels()]:
        assert np.array_equal(ref.hue(img, hue), np.asarray(pil_hue(Image.fromarray(img), hue)))


def test_blur_equals_pillow():
    sigmas = list(ref.SENSITIVE_SIGMAS) + [0.1, 2.0] + [float(s) for s in _rng(4).uniform(0.1, 2.0, 64).astype(np.float32)]
    radii = set()
    for img in _images():
        pim = Image.fromarray(img)
        for s in sigmas:
            radii.add(ref.box_params(s)[0])
            assert np.array_equal(ref.gaussian_blur(img, s), np.asarray(pim.filter(ImageFilter.GaussianBlur(radius=s)))), s
    assert radii == {0, 1}                                       # "for sigma <= 2, r <= 1", and both occur
    for shape in ((1, 9), (9, 1), (5, 7), (1, 1), (2, 3)):       # narrower than the blur reaches
        img = _rng(5).integers(0, 256, shape + (3,), dtype=np.uint8)
        for s in (0.1, 0.3, 1.0, 1.7320508, 2.0):
            assert np.array_equal(ref.gaussian_blur(img, s), np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius=s)))), (shape, s)


def test_solarize_and_grayscale_equal_pillow():
    for img in _images():
        pim = Image.fromarray(img)
        assert np.array_equal(ref.solarize(img), np.asarray(ImageOps.solarize(pim, 128)))
        assert np.array_equal(ref.grayscale(img), np.asarray(pim.convert("L").convert("RGB")))       # torchvision to_grayscale(img, 3)


def test_whole_chains_in_all_24_orders_equal_pillow():
    imgs = _images()
    for k, order in enumerate(itertools.permutations(range(4))):
        img = imgs[k % 2]
        factors = (FACTORS[k % 5], FACTORS[(k + 2) % 5], FACTORS[(k + 4) % 5], ref.HUES[k % 7])
        gray, sigma, sol = k % 3 == 0, ref.SIGMAS[k % 9], k % 2 == 0
        pim = Image.fromarray(img)
        for op in order:
            pim = PIL_OPS[op](pim, factors[op])
        if gray:
            pim = pim.convert("L").convert("RGB")
        if sigma is not None:
            pim = pim.filter(ImageFilter.GaussianBlur(radius=sigma))
        if sol:
            pim = ImageOps.solarize(pim, 128)
        got = ref.photometric(img, (order,) + factors + (gray, sigma, sol))
        assert np.array_equal(got, np.asarray(pim)), order


def test_draws_come_in_the_written_order():
    from mfvit.input_pipeline import AUG1, AUG2, GpuTransform, Photometric
    assert AUG1 == Photometric(0.8, 0.4, 0.4, 0.2, 0.1, 0.2, 1.0, (0.1, 2.0), 0.0)
    assert AUG2 == Photometric(0.8, 0.4, 0.4, 0.2, 0.1, 0.2, 0.1, (0.1, 2.0), 0.2)
    tf = GpuTransform("imagenet", img_size=224, mocov3=True, photometric=(AUG1, AUG2), device="cpu")
    sizes = [(320, 390), (90, 400), (256, 256)] * 6
    got = tf.sample_view_pairs(len(sizes), torch.Generator().manual_seed(31), sizes)
    g = torch.Generator().manual_seed(31)
    uni = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=g))
    rand = lambda: torch.rand(1, generator=g)
    seen = set()
    for (h, w), pair in zip(sizes, got):
        for recipe, view in zip((AUG1, AUG2), pair):
            box = GpuTransform.resized_crop_box(h, w, (0.08, 1.0), g)                      # 1
            order = b = c = s = hu = None
            if recipe.jitter_p >= float(rand()):                                           # 2
                order = tuple(torch.randperm(4, generator=g).tolist())                     # 3
                b, c, s, hu = uni(0.6, 1.4), uni(0.6, 1.4), uni(0.8, 1.2), uni(-0.1, 0.1)
            gray = bool(rand() < recipe.gray_p)                                            # 4
            sigma = uni(0.1, 2.0) if recipe.blur_p >= float(rand()) else None              # 5, 6
            sol = recipe is AUG2 and recipe.solarize_p >= float(rand())                    # 7
            flip = bool(rand() < 0.5)                                                      # 8
            assert view == (flip, 0.0, 0, 0, box, (order, b, c, s, hu, gray, sigma, sol))
            seen.add((order is None, gray, sigma is None, sol))
    assert len(seen) >= 6                                       # the draws took both branches of the optional steps
    assert all(q[5].sigma is not None and not q[5].solarize for q, _ in got)               # aug1: blur p = 1.0, no solarize
    # a chain without a recipe draws exactly what it drew before: box, flip, angle
    plain = GpuTransform("data", img_size=224, rotate=10, mocov3=True, device="cpu")
    got = plain.sample_params(3, torch.Generator().manual_seed(7), sizes[:3])
    g = torch.Generator().manual_seed(7)
    for (h, w), p in zip(sizes, got):
        box = GpuTransform.resized_crop_box(h, w, (0.08, 1.0), g)
        assert p == (bool(rand() < 0.5), uni(-10.0, 10.0), 0, 0, box)


def test_mutations_are_caught_by_the_gpu_tests_inputs():
    """Each deliberate error changes the expected output of the GPU test's own batch - at every size where it can show (a clamp at the
    tile edge needs a frame of more than one tile)."""
    for size in ref.SIZES:
        want = ref.reference(size)
        for m in ref.MUTATIONS:
            bad = ref.reference(size, m)
            hit = int((bad != want).any(axis=(1, 2, 3)).sum())
            if m == "tile_clamp" and size <= ref.TILE:
                assert hit == 0
            else:
                assert hit >= 5, (size, m, hit)
    # the double box weight shows at the rounding-sensitive sigmas themselves
    assert any(ref.box_params(s) != ref.box_params(s, "ww_double") for s in ref.SENSITIVE_SIGMAS)


def test_host_terms_descriptor_and_abi():
    from mfvit import _lib
    from mfvit.input_pipeline import MAX_BOX_RADIUS, NORMALIZE, GpuTransform, PhotoParams, box_blur_terms, photo_descriptor
    for s in list(ref.SENSITIVE_SIGMAS) + [0.1, 2.0, 1.4142134, 1.42, 2.4494896]:
        assert box_blur_terms(s) == ref.box_params(s) and box_blur_terms(s)[0] <= MAX_BOX_RADIUS
    assert box_blur_terms(2.4494898)[0] == 2                     # the first float32 sigma beyond the tile's halo
    assert NORMALIZE["imagenet"] == (ref.MEAN, ref.STD)
    d, r = photo_descriptor(PhotoParams((3, 1, 0, 2), 0.6, 1.0, 1.4, -0.1, True, 1.7320508, True))
    assert d[0] == 4 | 2 << 4 | 1 << 8 | 3 << 12 and d[4] == (-25) & 255 and d[5] == 7 and r == 1
    assert [np.int32(v).view(np.float32) for v in d[1:4]] == [np.float32(0.6), np.float32(1.0), np.float32(1.4)]
    assert tuple(d[6:9]) == ref.box_params(1.7320508) and not d[9:].any()
    d, r = photo_descriptor(PhotoParams(None, None, None, None, None, False, None, False))
    assert d[0] == 0 and d[5] == 0 and r == 0
    with pytest.raises(_lib.MfvitError):
        GpuTransform("imagenet", mocov3=False, photometric=PhotoParams)
    with pytest.raises(_lib.MfvitError):
        photo_descriptor(PhotoParams((0, 1, 2, 2), 1.0, 1.0, 1.0, 0.0, False, None, False))
    text = open(os.path.join(ROOT, "include", "mfvit.h")).read()
    for name in ("mfvit_input_photometric", "mfvit_input_photometric_workspace_bytes"):
        assert f" {name}(" in text and name in _lib.SIGNATURES
    h = _lib.lib()
    assert h.mfvit_abi_version() == 5                            # additive
    assert h.mfvit_input_photometric_workspace_bytes(3, 40) == 256 + 3 * 40 * 40 * 4
    assert h.mfvit_input_photometric_workspace_bytes(0, 40) == 0
    assert h.mfvit_input_photometric(1, 1, 1, 1, 1, 40, 2, 1, 1, 1, 1, None) == -38     # a box radius beyond the tile: refused before any HIP call
