"""GPU: the MoCo-v3 aug1 / aug2 chains through GpuTransform(photometric=...), bit-exact on the float32 output against
tests/photometric_ref.py (itself pinned against the installed Pillow in tests/test_photometric_cpu.py)."""
import numpy as np
import pytest
import torch

import photometric_ref as ref
from oracle import ref_input

pytestmark = pytest.mark.gpu


def _tf(size, recipes=None):
    from mfvit.input_pipeline import AUG1, GpuTransform
    return GpuTransform("imagenet", img_size=size, mocov3=True, photometric=recipes or AUG1)


def _mismatch(got, want):
    bad = (got != want).any(axis=(1, 2, 3))
    return [(int(k), int((got[k] != want[k]).sum()), float(np.abs(got[k] - want[k]).max())) for k in np.nonzero(bad)[0]]


@pytest.mark.parametrize("size", ref.SIZES)
def test_mixed_batch_bit_exact(size):
    """One launch over ref.samples(): the 24 operation orders, factors on both sides of 1 and exactly 1, gray, blur off / r = 0 / r = 1 /
    the rounding-sensitive sigmas, solarize, jitter off, flip, boxes on the image border - every sample with its own descriptor."""
    imgs, smp = ref.images(), ref.samples()
    got = _tf(size)([imgs[s] for s, *_ in smp], [(flip, 0.0, 0, 0, box) for _, flip, box, _ in smp], photo=[p for *_, p in smp]).cpu().numpy()
    want = ref.reference(size)
    assert got.shape == want.shape and got.dtype == want.dtype
    print(size, "mismatching samples (index, elements, max abs):", _mismatch(got, want))
    assert np.array_equal(got, want)


def test_descriptors_do_not_leak_between_samples():
    """The same samples in reverse order and in one-sample launches give the same images."""
    imgs, smp = ref.images(), ref.samples()[::-1][:12]
    want = ref.reference(40)[::-1][:12]
    tf = _tf(40)
    got = tf([imgs[s] for s, *_ in smp], [(flip, 0.0, 0, 0, box) for _, flip, box, _ in smp], photo=[p for *_, p in smp]).cpu().numpy()
    assert np.array_equal(got, want)
    for k in (0, 5, 11):
        s, flip, box, photo = smp[k]
        assert np.array_equal(tf([imgs[s]], [(flip, 0.0, 0, 0, box)], photo=[photo]).cpu().numpy()[0], want[k])


def test_two_views_aug1_aug2_from_a_seeded_generator():
    from mfvit.input_pipeline import AUG1, AUG2
    imgs = ref.images() * 4
    tf = _tf(40, (AUG1, AUG2))
    pairs = tf.sample_view_pairs(len(imgs), torch.Generator().manual_seed(5), [im.shape[:2] for im in imgs])
    q, k = tf.two_views(imgs, generator=torch.Generator().manual_seed(5))
    q, k = q.cpu().numpy(), k.cpu().numpy()
    assert q.shape == k.shape == (len(imgs), 3, 40, 40)
    for i, (im, (pq, pk)) in enumerate(zip(imgs, pairs)):
        assert pq[5].sigma is not None and not pq[5].solarize                     # aug1: blur p = 1.0, no solarize
        for got, (flip, _, _, _, box, photo) in ((q[i], pq), (k[i], pk)):
            assert np.array_equal(got, ref.transform_photo(im, box, 40, flip, tuple(photo), ref.MEAN, ref.STD)), i
    assert any(pk[5].solarize for _, pk in pairs) and any(pk[5].sigma is None for _, pk in pairs) and any(pk[5].sigma for _, pk in pairs)
    assert any(p[5].order is None for pr in pairs for p in pr) and any(p[5].gray for pr in pairs for p in pr)
    # explicit draws through photo= give the same views
    q2, k2 = tf.two_views(imgs, [(pq[:5], pk[:5]) for pq, pk in pairs], photo=[(pq[5], pk[5]) for pq, pk in pairs])
    assert np.array_equal(q2.cpu().numpy(), q) and np.array_equal(k2.cpu().numpy(), k)


def test_one_sample_at_224():
    img = ref.images()[0]
    photo = ((2, 1, 3, 0), 1.17, 0.6, 1.4, -0.1, False, 1.7320508, True)
    got = _tf(224)([img], [(True, 0.0, 0, 0, (0, 5, 40, 50))], photo=[photo]).cpu().numpy()
    assert np.array_equal(got[0], ref.transform_photo(img, (0, 5, 40, 50), 224, True, photo, ref.MEAN, ref.STD))


def test_plain_mocov3_chain_is_unchanged_and_large_radius_is_refused():
    from mfvit import _lib
    from mfvit.input_pipeline import NORMALIZE, GpuTransform
    imgs = ref.images()
    tf = GpuTransform("data", img_size=40, rotate=10, mocov3=True)
    ps = tf.sample_params(4, torch.Generator().manual_seed(3), [im.shape[:2] for im in imgs])
    got = tf(imgs, ps).cpu().numpy()
    for k, (im, (flip, angle, _, _, box)) in enumerate(zip(imgs, ps)):
        assert np.array_equal(got[k], ref_input.transform_mocov3(im, box, 40, flip, angle, *NORMALIZE["data"])), k
    with pytest.raises(_lib.MfvitError, match="-38"):              # r = 2: beyond the blur tile's halo
        _tf(40)(imgs[:1], [(False, 0.0, 0, 0, (0, 0, 40, 56))], photo=[(None, None, None, None, None, False, 2.5, False)])
