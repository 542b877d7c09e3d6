"""CPU: host half of the aspect-preserving input pipeline (GpuTransform(maintain_ratio=True), two_views) - resized frame sizes,
non-square rotation terms against the installed Pillow, torchvision's draw order, and the argument checks."""
import numpy as np
import pytest
import torch
from PIL import Image

from mfvit._lib import MfvitError
from mfvit.input_pipeline import GpuTransform, resized_size, rotation_terms


def _tv_resized(h, w, size):
    """torchvision _compute_resized_output_size for an int size (no max_size), restated: (new_h, new_w)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


# (h, w) of the source -> (Sh, Sw) of Resize(256)
FRAMES = [((390, 320), (312, 256)),      # portrait
          ((320, 390), (256, 312)),      # landscape (the CheXpert-small shape)
          ((512, 512), (256, 256)),      # square
          ((256, 300), (256, 300)),      # already at the short side: not resampled
          ((100, 80), (320, 256)),       # upscaled
          ((257, 511), (256, 509)),      # odd sizes
          ((224, 1024), (256, 1170)),    # extreme aspect ratio
          ((1024, 224), (1170, 256))]


@pytest.mark.parametrize("src,want", FRAMES)
def test_frame_sizes(src, want):
    assert resized_size(*src, 256) == want == _tv_resized(*src, 256)
    tf = GpuTransform(img_size=256, crop=224, maintain_ratio=True)
    assert tf.frame(*src) == want
    assert GpuTransform(img_size=256, crop=224).frame(*src) == (256, 256)    # the default keeps Resize((S, S))


def test_frame_sizes_random():
    rng = np.random.Generator(np.random.PCG64(3))
    for h, w in rng.integers(1, 4000, (500, 2)):
        for size in (224, 256, 384):
            assert resized_size(int(h), int(w), size) == _tv_resized(int(h), int(w), size)


def _rotate_host(f, angle):
    """The rotation the kernel applies with rotation_terms' output, as a small numpy NEAREST gather (fill 0)."""
    h, w = f.shape[:2]
    mode, t = rotation_terms(angle, w, h)
    if mode == 0:
        return f.copy()
    if mode == 3:
        return f[::-1, ::-1]
    if mode in (2, 4):
        assert w == h
        return np.rot90(f, 1 if mode == 2 else 3)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    xx = (t[2] + t[1] * ys + t[0] * xs) >> 16
    yy = (t[5] + t[4] * ys + t[3] * xs) >> 16
    ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
    out = np.zeros_like(f)
    out[ok] = f[yy[ok], xx[ok]]
    return out


@pytest.mark.parametrize("hw", [(256, 312), (312, 256), (37, 53), (256, 256), (1170, 256)])
@pytest.mark.parametrize("angle", [0.0, 3.7, -3.7, 9.99, -9.99, 45.0, 90.0, 180.0, 270.0])
def test_rotation_terms_non_square_bit_exact(hw, angle):
    f = np.random.Generator(np.random.PCG64(hw[0] * 7 + hw[1])).integers(0, 256, (*hw, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(f).rotate(angle, Image.NEAREST, expand=False, fillcolor=0))
    assert np.array_equal(_rotate_host(f, angle), want)


def test_rotation_terms_fast_paths():
    assert rotation_terms(90.0, 256) == rotation_terms(90.0, 256, 256) and rotation_terms(90.0, 256)[0] == 2
    assert rotation_terms(270.0, 256)[0] == 4 and rotation_terms(180.0, 312, 256)[0] == 3 and rotation_terms(-360.0, 312, 256)[0] == 0
    assert rotation_terms(90.0, 312, 256)[0] == 1 and rotation_terms(-90.0, 256, 312)[0] == 1   # Pillow transposes only square frames


def _replay(g, frames, C, rotate):
    """torchvision: RandomHorizontalFlip, RandomRotation.get_params, RandomCrop.get_params, in that order, per frame."""
    out = []
    for fh, fw in frames:
        flip = bool(torch.rand(1, generator=g) < 0.5)
        angle = float(torch.empty(1).uniform_(float(-rotate), float(rotate), generator=g).item())
        if fh < C or fw < C:
            raise ValueError
        if fw == C and fh == C:
            i = j = 0
        else:
            i = torch.randint(0, fh - C + 1, size=(1,), generator=g).item()
            j = torch.randint(0, fw - C + 1, size=(1,), generator=g).item()
        out.append((flip, angle, i, j))
    return out


def test_sample_params_draw_order():
    sizes = [(390, 320), (320, 390), (224, 224), (600, 224), (300, 300), (224, 224), (100, 80)]
    tf = GpuTransform(img_size=224, crop=224, rotate=10, maintain_ratio=True)
    frames = [tf.frame(*s) for s in sizes]
    assert frames[2] == frames[5] == (224, 224) and frames[4] == (224, 224)        # RandomCrop draws nothing for these
    got = tf.sample_params(len(sizes), torch.Generator().manual_seed(4), sizes)
    assert got == _replay(torch.Generator().manual_seed(4), frames, 224, 10)
    assert got[2][2:] == (0, 0) and got[1][2] == 0 and got[0][3] == 0
    tf = GpuTransform(img_size=256, crop=224, rotate=7, maintain_ratio=True)
    g = torch.Generator().manual_seed(5)
    got = tf.sample_params(len(sizes), g, sizes)
    g2 = torch.Generator().manual_seed(5)
    assert got == _replay(g2, [tf.frame(*s) for s in sizes], 224, 7)
    assert torch.equal(g.get_state(), g2.get_state())
    assert all(0 <= i <= fh - 224 and 0 <= j <= fw - 224 for (_, _, i, j), (fh, fw) in zip(got, map(lambda s: tf.frame(*s), sizes)))
    # crop=0: no RandomCrop in the chain, so nothing is drawn for it
    tf = GpuTransform(img_size=256, crop=0, rotate=7, maintain_ratio=True)
    g = torch.Generator().manual_seed(6)
    got = tf.sample_params(3, g, sizes[:3])
    g2 = torch.Generator().manual_seed(6)
    want = [(bool(torch.rand(1, generator=g2) < 0.5), float(torch.empty(1).uniform_(-7.0, 7.0, generator=g2)), 0, 0) for _ in range(3)]
    assert got == want and torch.equal(g.get_state(), g2.get_state())


def test_two_view_draw_order():
    sizes = [(390, 320), (224, 224), (320, 390)]
    tf = GpuTransform(img_size=224, crop=224, rotate=10, maintain_ratio=True)
    pairs = tf.sample_view_pairs(3, torch.Generator().manual_seed(8), sizes)
    frames = [tf.frame(*s) for s in sizes]
    flat = _replay(torch.Generator().manual_seed(8), [f for f in frames for _ in range(2)], 224, 10)   # q0 k0 q1 k1 q2 k2
    assert [p for pair in pairs for p in pair] == flat
    assert pairs[1] == tuple(flat[2:4]) and pairs[0][0] != pairs[0][1]
    # the square path and the mocov3 path follow the same per-image q-then-k order
    sq = GpuTransform(img_size=256, crop=224, rotate=10)
    pairs = sq.sample_view_pairs(3, torch.Generator().manual_seed(9))
    assert [p for pair in pairs for p in pair] == sq.sample_params(6, torch.Generator().manual_seed(9))
    mo = GpuTransform(img_size=224, rotate=10, mocov3=True, maintain_ratio=True)
    pairs = mo.sample_view_pairs(3, torch.Generator().manual_seed(10), sizes)
    want = mo.sample_params(6, torch.Generator().manual_seed(10), [s for s in sizes for _ in range(2)])
    assert [p for pair in pairs for p in pair] == want


def test_center_crop_offsets_round_half_even():
    ev = GpuTransform(img_size=256, crop=224, training=False, maintain_ratio=True)
    sizes = [(512, 514), (512, 518), (320, 390), (390, 320), (256, 256)]
    assert [ev.frame(*s) for s in sizes] == [(256, 257), (256, 259), (256, 312), (312, 256), (256, 256)]
    assert ev.sample_params(5, None, sizes) == [(False, 0.0, 16, 16), (False, 0.0, 16, 18), (False, 0.0, 16, 44), (False, 0.0, 44, 16),
                                                (False, 0.0, 16, 16)]
    mo = GpuTransform(img_size=224, crop=224, training=False, mocov3=True, maintain_ratio=True)     # Resize(256) -> CenterCrop(224)
    assert mo.frame(320, 390) == (256, 312) and mo.sample_params(1, None, [(320, 390)]) == [(False, 0.0, 16, 44)]
    assert GpuTransform(img_size=224, training=True, mocov3=True, maintain_ratio=True).frame(320, 390) == (224, 224)


def _imgs(sizes):
    return [np.zeros((h, w, 3), np.uint8) for h, w in sizes]


def test_errors():
    with pytest.raises(MfvitError, match="crop larger"):
        GpuTransform(img_size=200, crop=224, maintain_ratio=True)
    tf = GpuTransform(img_size=256, crop=224, maintain_ratio=True)
    with pytest.raises(MfvitError, match="sizes"):
        tf.sample_params(2)
    with pytest.raises(MfvitError, match="crop offset"):       # offsets outside the image's own frame
        tf(_imgs([(320, 390)]), [(False, 0.0, 0, 89)])
    nc = GpuTransform(img_size=256, crop=0, maintain_ratio=True)
    with pytest.raises(MfvitError, match="cannot form one batch"):
        nc(_imgs([(320, 390), (390, 320)]), [(False, 0.0, 0, 0)] * 2)
    with pytest.raises(MfvitError, match="cannot form one batch"):
        nc.two_views(_imgs([(320, 390), (300, 300)]), [((False, 0.0, 0, 0),) * 2] * 2)
    p = (False, 0.0, 0, 0)
    for bad in ([(p, p)], [(p, p), (p,)], [(p, p), (p, p, p)], [(p, p), ((False, 0.0), p)], [p, p]):
        with pytest.raises(MfvitError, match="two_views params"):
            tf.two_views(_imgs([(320, 390), (390, 320)]), bad)
