"""GPU: the aspect-preserving input pipeline (GpuTransform(maintain_ratio=True): Resize(S), per-sample Sh x Sw frames) and MoCo's
two views, bit-exact against a Pillow chain built here: resize(BILINEAR) -> FLIP_LEFT_RIGHT -> rotate(NEAREST, fill 0) -> crop ->
ToTensor -> Normalize in float32."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import ref_input

pytestmark = pytest.mark.gpu


def _images(seed, sizes):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _pillow(im, frame, flip, angle, ij, out_hw, mean, std, box=None):
    """frame = (Sh, Sw) of the resize, out_hw = (h, w) of the crop window at ij = (i, j)."""
    x = Image.fromarray(im)
    if box is not None:
        i, j, h, w = box
        x = x.crop((j, i, j + w, i + h))
    x = x.resize((frame[1], frame[0]), Image.BILINEAR)
    if flip:
        x = x.transpose(Image.FLIP_LEFT_RIGHT)
    x = x.rotate(angle, Image.NEAREST, expand=False, fillcolor=0)
    x = x.crop((ij[1], ij[0], ij[1] + out_hw[1], ij[0] + out_hw[0]))
    a = np.asarray(x).astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    return (a - np.asarray(mean, np.float32).reshape(3, 1, 1)) / np.asarray(std, np.float32).reshape(3, 1, 1)


def _check(tf, imgs, params, got, C=None):
    C = tf.crop if C is None else C
    for k, (im, prm) in enumerate(zip(imgs, params)):
        box = prm[4] if len(prm) > 4 else None
        fr = tf.frame(*(box[2:] if box else im.shape[:2]))
        want = _pillow(im, fr, prm[0], prm[1], prm[2:4], (C, C) if isinstance(C, int) else C, tf.mean, tf.std, box)
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        assert np.array_equal(got[k], want), (k, im.shape, prm, np.abs(got[k] - want).max())


SIZES = [(390, 320), (320, 390), (512, 512), (256, 300), (100, 80), (257, 511), (224, 1024), (1024, 224), (2000, 1700), (1700, 2000)]


@pytest.mark.parametrize("img_type", ["CheXpert-v1.0-small", "CheXpert_Enh", "data", "Train_Mix"])
def test_training_chain_bit_exact(img_type):
    from mfvit.input_pipeline import GpuTransform
    tf = GpuTransform(img_type, img_size=256, crop=224, rotate=10, training=True, maintain_ratio=True)
    imgs = _images(21, SIZES)
    angles = [0.0, 3.7, -9.99, 90.0, 270.0, 180.0, 45.0, -3.7, 90.0, 270.0]
    params = []
    for k, im in enumerate(imgs):
        fh, fw = tf.frame(*im.shape[:2])
        i = (0, fh - 224)[k % 2]                       # both ends of each axis
        j = (0, fw - 224)[(k // 2) % 2]
        params.append((k % 3 == 1, angles[k], i, j))
    got = tf(imgs, params).cpu().numpy()
    assert got.shape == (len(imgs), 3, 224, 224)
    _check(tf, imgs, params, got)
    # the far corner of every frame and the opposite flips
    params = [(not f, -a, tf.frame(*im.shape[:2])[0] - 224, tf.frame(*im.shape[:2])[1] - 224) for im, (f, a, _, _) in zip(imgs, params)]
    _check(tf, imgs, params, tf(imgs, params).cpu().numpy())


def test_sampled_params_and_no_crop():
    from mfvit.input_pipeline import GpuTransform
    tf = GpuTransform("data", img_size=256, crop=224, rotate=10, training=True, maintain_ratio=True)
    imgs = _images(22, SIZES[:8])
    ps = tf.sample_params(len(imgs), torch.Generator().manual_seed(3), [im.shape[:2] for im in imgs])
    got = tf(imgs, generator=torch.Generator().manual_seed(3)).cpu().numpy()
    _check(tf, imgs, ps, got)
    # crop=0: the whole resized frame; same-size sources give one (possibly non-square) batch
    nc = GpuTransform("CheXpert-v1.0-small", img_size=256, crop=0, rotate=10, training=True, maintain_ratio=True)
    imgs = _images(23, [(320, 390)] * 3)
    params = [(True, 4.5, 0, 0), (False, 90.0, 0, 0), (False, 0.0, 0, 0)]
    got = nc(imgs, params).cpu().numpy()
    assert got.shape == (3, 3, 256, 312)
    _check(nc, imgs, params, got, C=(256, 312))


def test_eval_chain():
    from mfvit.input_pipeline import GpuTransform
    ev = GpuTransform("Train_Mix", img_size=256, crop=224, training=False, maintain_ratio=True)
    imgs = _images(24, [(512, 514), (512, 518), (320, 390), (390, 320), (256, 256)])
    ps = ev.sample_params(len(imgs), None, [im.shape[:2] for im in imgs])
    assert ps[0][2:] == (16, 16) and ps[1][2:] == (16, 18)                  # (257-224)/2 = 16.5 -> 16, (259-224)/2 = 17.5 -> 18
    got = ev(imgs).cpu().numpy()
    _check(ev, imgs, ps, got)
    mo = GpuTransform("data", img_size=224, crop=224, training=False, mocov3=True, maintain_ratio=True)     # Resize(256) -> CenterCrop(224)
    ps = mo.sample_params(len(imgs), None, [im.shape[:2] for im in imgs])
    got = mo(imgs).cpu().numpy()
    assert mo.frame(320, 390) == (256, 312)
    _check(mo, imgs, ps, got)
    # mocov3 training keeps RandomResizedCrop's square output whatever maintain_ratio says
    tr = GpuTransform("data", img_size=224, training=True, mocov3=True, maintain_ratio=True)
    ps = tr.sample_params(len(imgs), torch.Generator().manual_seed(2), [im.shape[:2] for im in imgs])
    got = tr(imgs, ps).cpu().numpy()
    for k, (im, (f, a, _, _, box)) in enumerate(zip(imgs, ps)):
        assert np.array_equal(got[k], ref_input.transform_mocov3(im, box, 224, f, a, tr.mean, tr.std)), k


def test_two_views(monkeypatch):
    from mfvit import input_pipeline as ip
    tf = ip.GpuTransform("CheXpert-v1.0-small", img_size=256, crop=224, rotate=10, training=True, maintain_ratio=True)
    imgs = _images(25, SIZES[:6])
    pairs = tf.sample_view_pairs(len(imgs), torch.Generator().manual_seed(11), [im.shape[:2] for im in imgs])
    uploads = []
    real = torch.from_numpy

    def spy(a):
        if a.dtype == np.uint8:
            uploads.append(a.size)
        return real(a)
    monkeypatch.setattr(ip.torch, "from_numpy", spy)
    q, k = tf.two_views(imgs, pairs)
    monkeypatch.undo()
    assert uploads == [sum(im.size for im in imgs)]                          # every source once, for both views
    assert q.shape == k.shape == (len(imgs), 3, 224, 224) and q.is_contiguous() and k.is_contiguous()
    q1 = tf(imgs, [p[0] for p in pairs])
    k1 = tf(imgs, [p[1] for p in pairs])
    assert torch.equal(q, q1) and torch.equal(k, k1)
    _check(tf, imgs, [p[0] for p in pairs], q.cpu().numpy())
    _check(tf, imgs, [p[1] for p in pairs], k.cpu().numpy())
    # default draws: the same generator state gives the same pairs; the two views differ
    q2, k2 = tf.two_views(imgs, generator=torch.Generator().manual_seed(11))
    assert torch.equal(q2, q) and torch.equal(k2, k)
    assert all(not torch.equal(q[s], k[s]) for s in range(len(imgs)))
    # the square path and MoCo's RandomResizedCrop views
    for t in (ip.GpuTransform("data", img_size=256, crop=224, training=True),
              ip.GpuTransform("data", img_size=224, training=True, mocov3=True, maintain_ratio=True)):
        pairs = t.sample_view_pairs(len(imgs), torch.Generator().manual_seed(12), [im.shape[:2] for im in imgs])
        q, k = t.two_views(imgs, pairs)
        assert torch.equal(q, t(imgs, [p[0] for p in pairs])) and torch.equal(k, t(imgs, [p[1] for p in pairs]))


def test_random_sizes_batch_128():
    """A loader-sized batch: 128 sources of 256..2048 on each axis, every sample against Pillow (the out-of-bounds check)."""
    from mfvit.input_pipeline import GpuTransform
    rng = np.random.Generator(np.random.PCG64(26))
    sizes = [tuple(int(v) for v in rng.integers(256, 2049, 2)) for _ in range(128)]
    imgs = _images(27, sizes)
    tf = GpuTransform("CheXpert_Enh", img_size=256, crop=224, rotate=10, training=True, maintain_ratio=True)
    ps = tf.sample_params(128, torch.Generator().manual_seed(28), sizes)
    ps = [(f, (90.0, 270.0, 180.0)[k % 3] if k % 8 == 0 else a, i, j) for k, (f, a, i, j) in enumerate(ps)]
    got = tf(imgs, ps).cpu().numpy()
    assert np.isfinite(got).all()
    _check(tf, imgs, ps, got)


def test_square_path_unchanged():
    """maintain_ratio=False still equals oracle/ref_input.py bit for bit, through GpuTransform and through the square entry point
    mfvit_input_transform with descriptors whose slot 17 is zero."""
    from mfvit import input_pipeline as ip
    from mfvit._lib import check, lib, ptr, stream
    sizes = [(320, 390), (390, 320), (256, 256), (100, 80), (2000, 1700)]
    imgs = _images(29, sizes)
    params = [(False, 0.0, 0, 0), (True, 90.0, 32, 32), (False, 270.0, 5, 31), (True, 180.0, 16, 0), (False, -7.25, 32, 1)]
    tf = ip.GpuTransform("data", img_size=256, crop=224, rotate=10, training=True)
    got = tf(imgs, params)
    for k, (im, (f, a, i, j)) in enumerate(zip(imgs, params)):
        assert np.array_equal(got[k].cpu().numpy(), ref_input.transform(im, 256, f, a, (i, j), 224, tf.mean, tf.std)), k
    desc = np.zeros((len(imgs), 20), dtype=np.int64)
    tabs, pos, off = [], 0, 0
    for s, (im, (f, a, i, j)) in enumerate(zip(imgs, params)):
        H, W = im.shape[:2]
        ksx, tx = ip.axis_table(W, 256)
        ksy, ty = ip.axis_table(H, 256)
        tabs += [tx.reshape(-1), ty.reshape(-1)]
        mode, terms = ip.rotation_terms(a, 256)
        desc[s] = [off, H, W, pos, pos + tx.size, ksx, ksy, int(f), mode, *terms, (i << 32) | j, W * 3, 0, 0, 0]
        pos += tx.size + ty.size
        off += im.size
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
    dsc = torch.from_numpy(desc).cuda()
    tab = torch.from_numpy(np.concatenate(tabs)).cuda()
    out = torch.empty(len(imgs), 3, 224, 224, device="cuda")
    mean = (ctypes.c_float * 3)(*tf.mean)
    std = (ctypes.c_float * 3)(*tf.std)
    check(lib().mfvit_input_transform(ptr(src), ptr(dsc), ptr(tab), len(imgs), 256, 224, ctypes.cast(mean, ctypes.c_void_p),
                                      ctypes.cast(std, ctypes.c_void_p), ptr(out), stream()), "mfvit_input_transform")
    torch.cuda.synchronize()
    assert torch.equal(out, got)
