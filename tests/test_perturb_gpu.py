"""The perturbation test for relevance maps on the GPU (include/mfvit.h: mfvit_patch_rank, mfvit_patch_perturb, mfvit_perturb_score;
csrc/perturb.hip; mfvit.perturb) against the numpy / float64 restatements of tests/perturb_ref.py.

Ranks and masked images are exact (integers; moves and fills).  The score's sums are held to 1e-12 relative.  That bound is derived, not
measured: a double exp a few ulp off over at most 64 + 16 terms is about 1e-14; 1e-12 leaves a margin of a hundred and sits four decades
below f32 epsilon, so a single-precision exp or sum fails it."""
import importlib

import numpy as np
import pytest
import torch

import perturb_ref as R
from conftest import rng_tensor
from oracle import ref_fusion, ref_vit

DEV = "cuda:0"
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"
SUM_TOL = 1e-12
POISON = 0x5A5A5A5A


def _p():
    from mfvit import perturb
    return perturb


def _lib():
    from mfvit import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ 1. rank
@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 196, 197, 576, 1025, 8192])
def test_rank_is_exactly_the_reference_inside_a_poisoned_buffer(P):
    B, pad, guard = 3, 5, 64
    L = _lib()
    for k, kind in enumerate(R.RANK_KINDS):
        rel = R.rank_inputs(kind, B, P, seed=11 * P + k)
        # (the pairwise reference costs O(P^2) memory; tests/test_perturb_cpu.py shows the argsort form equal to it)
        ref = R.ref_rank(rel) if P <= 1025 else R.inverse_argsort_rank(rel)
        # the row stride is P + pad on the odd kinds; the columns behind a row hold values that would move the ranks if they were read
        ld = P + pad if k % 2 else P
        src = torch.full((B, ld), 1e30, dtype=torch.float32)
        src[:, :P] = torch.from_numpy(rel)
        src = src.to(DEV)
        buf = torch.full((guard + B * P + guard,), POISON, dtype=torch.int32, device=DEV)
        L.check(L.lib().mfvit_patch_rank(src.data_ptr(), ld, buf.data_ptr() + 4 * guard, B, P, _stream()), "mfvit_patch_rank")
        host = buf.cpu().numpy()
        assert (host[:guard] == POISON).all() and (host[guard + B * P:] == POISON).all(), f"{kind}: a neighbour of the output was written"
        msg = R.rank_mismatch(host[guard:guard + B * P].reshape(B, P), ref)
        assert msg is None, f"{kind}, P = {P}, ld = {ld}: {msg}"
        # the wrapper: the same ranks from a strided view, from (B, gh, gw) and from float64
        got = _p().patch_rank(src[:, :P])
        assert got.dtype == torch.int32 and got.shape == (B, P) and R.rank_mismatch(got.cpu().numpy(), ref) is None
    if P == 576:
        rel = R.rank_inputs("normal", B, P, seed=3)
        t = torch.from_numpy(rel).to(DEV)
        ref = R.ref_rank(rel)
        assert R.rank_mismatch(_p().patch_rank(t.view(B, 24, 24)).cpu().numpy(), ref) is None
        assert R.rank_mismatch(_p().patch_rank(t.double()).cpu().numpy(), ref) is None


# ------------------------------------------------------------------------------------------------ 2. mask
def _mask_case(B, C, H, W, seed):
    P = (H // 16) * (W // 16)
    g = np.random.Generator(np.random.PCG64(seed))
    img = g.standard_normal((B, C, H, W)).astype(np.float32)
    rank = np.stack([g.permutation(P) for _ in range(B)]).astype(np.int32)
    ks = [0, 1, P - 1, P, P // 2]
    ranges = np.concatenate([_p().ranges_for(P, ks, mode).numpy() for mode in ("positive", "negative", "insertion")])
    fill = (0.5 + np.arange(C, dtype=np.float32)) * np.float32(-1.25)             # non-zero, different per channel
    return img, rank, ranges, fill


def _run_mask(img, rank, ranges, fill, offset_bytes):
    """mfvit_patch_perturb with img and out `offset_bytes` behind their allocations and out between NaN guard bands: (out, guards intact)."""
    L = _lib()
    B, C, H, W = img.shape
    S, n, guard, off = len(ranges), img.size, 256, offset_bytes // 4
    src = torch.full((off + n,), float("nan"), dtype=torch.float32, device=DEV)
    src[off:] = torch.from_numpy(img).reshape(-1).to(DEV)
    dst = torch.full((off + guard + S * n + guard,), float("nan"), dtype=torch.float32, device=DEV)
    rk, st, fl = torch.from_numpy(rank).to(DEV), torch.from_numpy(ranges).to(DEV), torch.from_numpy(fill).to(DEV)
    L.check(L.lib().mfvit_patch_perturb(src.data_ptr() + 4 * off, rk.data_ptr(), st.data_ptr(), fl.data_ptr(), dst.data_ptr() + 4 * (off + guard),
                                        B, C, H, W, S, _stream()), "mfvit_patch_perturb")
    host = dst.cpu().numpy()
    intact = bool(np.isnan(host[:off + guard]).all() and np.isnan(host[off + guard + S * n:]).all())
    return host[off + guard:off + guard + S * n].reshape(S, B, C, H, W), intact


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (3, 3, 32, 48), (2, 1, 48, 32), (2, 3, 224, 224)])
def test_masked_batches_are_bit_exact_between_guard_bands(shape):
    img, rank, ranges, fill = _mask_case(*shape, seed=sum(shape))
    ref = R.ref_perturb(img, rank, ranges, fill)
    assert len(ranges) == 15
    got, intact = _run_mask(img, rank, ranges, fill, 16)                           # 16 bytes behind the allocation: the 16-byte path
    assert intact, "a guard band was written"
    assert np.array_equal(got, ref)
    again, _ = _run_mask(img, rank, ranges, fill, 16)
    assert again.tobytes() == got.tobytes()                                       # the same call twice: the same bits
    if shape != (2, 3, 224, 224):
        got4, intact4 = _run_mask(img, rank, ranges, fill, 4)                      # 4 bytes behind: the scalar path
        assert intact4 and np.array_equal(got4, ref)
    # the wrapper, with each form of fill
    p = _p()
    x, rk = torch.from_numpy(img).to(DEV), torch.from_numpy(rank).to(DEV)
    out = p.perturb_patches(x, rk, ranges.tolist(), fill.tolist())
    assert out.shape == (15,) + shape and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), ref)
    zero = p.perturb_patches(x, rk, torch.from_numpy(ranges).to(DEV))
    assert np.array_equal(zero.cpu().numpy(), R.ref_perturb(img, rank, ranges, np.zeros(shape[1], np.float32)))
    one = p.perturb_patches(x, rk, ranges[:2], 0.75)
    assert np.array_equal(one.cpu().numpy(), R.ref_perturb(img, rank, ranges[:2], np.full(shape[1], 0.75, np.float32)))


# ------------------------------------------------------------------------------------------------ 3. score
def _score_case(S, B, C, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    z = (g.standard_normal((S, B, C)) * 3).astype(np.float32)
    t = g.integers(0, C, size=B)
    for s in range(S):
        for b in range(0, B, 3):                                                   # exact ties at the maximum, the target among them or not
            z[s, b, g.integers(0, C, size=2)] = z[s, b].max() + np.float32(1.0)
    z[0, 0, 0], z[1, 0, C - 1] = 80.0, -80.0                                        # large magnitudes
    if B > 1:
        z[1, 1, :] = 80.0
        z[2, B - 1, 0] = -80.0
    z[3, B // 2, C // 2] = [np.inf, -np.inf, np.nan][seed % 3]                      # one non-finite row
    return z, t


def _score(z, t):
    S = z.shape[0]
    c, s, n = (torch.zeros(S, dtype=torch.int64, device=DEV), torch.zeros(S, 2, dtype=torch.float64, device=DEV),
               torch.zeros(S, dtype=torch.int64, device=DEV))
    _p().perturb_score(z, t, c, s, n)
    return c.cpu(), s.cpu(), n.cpu()


def _assert_score(got, ref, what):
    (c, s, n), (rc, rn, rs) = got, ref
    assert c.tolist() == rc and n.tolist() == rn, what
    for step in range(len(rc)):
        for q in range(2):
            a, b = float(s[step, q]), rs[step][q]
            print(f"[score {what}] step {step} sum {q}: got {a!r}, ref {b!r}, rel {abs(a - b) / max(abs(b), 1e-300):.2e}")
            assert abs(a - b) <= SUM_TOL * abs(b), (what, step, q, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, 16])
@pytest.mark.parametrize("B", [1, 7, 64, 300])
def test_score_counts_are_exact_and_sums_within_1e_12(B, C):
    z, t = _score_case(4, B, C, seed=100 * B + C)
    ref = R.ref_score(z, t)
    assert ref[1] == [0, 0, 0, 1]
    zt, tt = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
    _assert_score(_score(zt, tt), ref, f"B={B} C={C}")
    # a padded row stride, with a larger value than any logit behind every row
    wide = torch.full((4, B, C + 3), 1e30, dtype=torch.float32, device=DEV)
    wide[:, :, :C] = zt
    got = _score(wide[:, :, :C], tt)
    first = _score(zt, tt)
    assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]) and torch.equal(got[2], first[2])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [7, 64, 300])
def test_two_updates_equal_the_two_halves_added_in_order_bit_for_bit(B):
    p = _p()
    z, t = _score_case(4, B, 3, seed=B)
    zt, tt = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
    h = B // 2
    m = p.PerturbationMeter(4, fractions=(0, .25, .5, 1))
    m.update(zt[:, :h], tt[:h])
    m.update(zt[:, h:], tt[h:])
    a, b = _score(zt[:, :h].contiguous(), tt[:h]), _score(zt[:, h:].contiguous(), tt[h:])
    c, n, s = (v.cpu() for v in m._views())
    assert torch.equal(c, a[0] + b[0]) and torch.equal(n, a[2] + b[2])
    assert torch.equal(s, (torch.zeros(4, 2, dtype=torch.float64) + a[1]) + b[1])            # bit for bit
    again = p.PerturbationMeter(4)
    again.update(zt[:, :h], tt[:h])
    again.update(zt[:, h:], tt[h:])
    assert torch.equal(again._buf, m._buf)                                                  # the same bits on every run
    res = m.compute()
    ref = R.ref_score(z, t)
    assert res.n == B and res.nonfinite == ref[1] and res.accuracy == [k / B for k in ref[0]]
    assert res.mean_prob == [float(s[k, 0]) / B for k in range(4)] and res.mean_logit == [float(s[k, 1]) / B for k in range(4)]
    _assert_score((c, s, n), ref, f"two updates B={B}")


# ------------------------------------------------------------------------------------------------ 4. end to end, one encoder
def _encoder(seed=7, depth=2):
    import vits
    m = vits.vit_small(num_classes=3, depth=depth)
    m.load_state_dict(ref_vit.seeded_params(seed, num_classes=3, depth=depth))
    return m.to(DEV)


@pytest.fixture(scope="module")
def single():
    m = _encoder()
    B = 3
    img = rng_tensor(91, (B, 3, 224, 224))
    maps = rng_tensor(92, (B, 14, 14))
    return m, img, maps


def _forward(model, x):
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            return model(x.to(DEV))
    finally:
        model.train(was)


FRACTIONS = (0, .25, .5, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["positive", "negative", "insertion"])
def test_single_encoder_logits_are_the_models_on_the_reference_masks(single, mode):
    p = _p()
    m, img, maps = single
    B, P = 3, 196
    x, mp = img.to(DEV), maps.to(DEV)
    target = torch.tensor([2, 0, 1])
    meter, logits = p.perturbation_test(m, x, mp, target=target, fractions=FRACTIONS, mode=mode, max_batch=B, return_logits=True)
    assert logits.shape == (4, B, 3) and logits.dtype == torch.float32 and not logits.requires_grad
    ks = p.step_counts(P, FRACTIONS)
    assert ks == [0, 49, 98, 196]
    rank = p.patch_rank(mp).cpu().numpy()
    assert R.rank_mismatch(rank, R.ref_rank(maps.reshape(B, P).numpy())) is None
    masked = R.ref_perturb(img.numpy(), rank, p.ranges_for(P, ks, mode).tolist(), np.zeros(3, np.float32))
    for s in range(4):
        assert torch.equal(logits[s], _forward(m, torch.from_numpy(masked[s]))), f"step {s}"
    # the meter against float64 on those logits
    res = meter.compute()
    rc, rn, rs = R.ref_score(logits.cpu().numpy(), target.numpy())
    assert res.n == B and res.nonfinite == rn == [0] * 4 and res.accuracy == [c / B for c in rc]
    assert res.fractions == [k / P for k in ks]
    c, n, acc = (v.cpu() for v in meter._views())
    _assert_score((c, acc, n), (rc, rn, rs), f"e2e {mode}")
    assert res.mean_prob == [float(acc[s, 0]) / B for s in range(4)] and res.mean_logit == [float(acc[s, 1]) / B for s in range(4)]
    blank, clean = _forward(m, torch.zeros(B, 3, 224, 224)), _forward(m, img)
    if mode == "insertion":
        assert torch.equal(logits[3], clean) and torch.equal(logits[0], blank)
    else:
        assert torch.equal(logits[0], clean) and torch.equal(logits[3], blank)    # fraction 1, default fill: the all-zero image


@pytest.mark.gpu
def test_predicted_target_grouping_and_side_effects(single):
    p = _p()
    m, img, maps = single
    B = 3
    x, mp = img.to(DEV), maps.to(DEV)
    clean = _forward(m, img)
    # target None: the argmax of step 0
    m0, l0 = p.perturbation_test(m, x, mp, fractions=FRACTIONS, return_logits=True)
    m1, l1 = p.perturbation_test(m, x, mp, target=clean.argmax(dim=1), fractions=FRACTIONS, return_logits=True)
    assert torch.equal(l0, l1) and torch.equal(m0._buf, m1._buf)
    assert m0.compute().accuracy[0] == 1.0
    # ... and of the unperturbed image in insertion mode, whose step 0 hides everything
    m2 = p.perturbation_test(m, x, mp, fractions=FRACTIONS, mode="insertion")
    m3 = p.perturbation_test(m, x, mp, target=clean.argmax(dim=1).cpu(), fractions=FRACTIONS, mode="insertion")
    assert torch.equal(m2._buf, m3._buf) and m2.compute().accuracy[3] == 1.0
    # max_batch = 2 B: two steps per forward, the logits of the model at that batch size
    _, lg = p.perturbation_test(m, x, mp, target=1, fractions=FRACTIONS, max_batch=2 * B + 1, return_logits=True)
    masked = p.perturb_patches(x, p.patch_rank(mp), p.ranges_for(196, p.step_counts(196, FRACTIONS), "positive"))
    for s0 in (0, 2):
        assert torch.equal(lg[s0:s0 + 2].reshape(2 * B, 3), _forward(m, masked[s0:s0 + 2].flatten(0, 1)))
    # a meter passed in accumulates; a map as (B, P) and a (B,) device target are taken
    meter = p.PerturbationMeter(4)
    for _ in range(2):
        assert p.perturbation_test(m, x, mp.view(B, 196), target=torch.tensor([2, 0, 1], device=DEV), fractions=FRACTIONS, meter=meter) is meter
    assert meter.n == 2 * B and meter.compute().n == 2 * B
    # no side effects: training mode with dropout rates would draw seeds if the forwards were not evaluation forwards
    import vits
    d = vits.vit_small(num_classes=3, depth=2, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1)
    d.load_state_dict(ref_vit.seeded_params(7, num_classes=3, depth=2))
    d = d.to(DEV).train()
    d(x).sum().backward()                                                         # a gradient arena exists
    d.zero_grad(set_to_none=True)
    arena = d._grad_arena
    snap = arena.clone()
    d.eval()
    with torch.no_grad():
        d.features3D(x)                                                           # (a feature cache entry: evaluation forwards keep one)
    d.train()
    cache = d._feat_cache
    assert cache is not None
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    _, ld = p.perturbation_test(d, x, mp, target=1, fractions=FRACTIONS, return_logits=True)
    torch.cuda.synchronize()
    assert d.training and all(mod.training for mod in d.modules())
    assert d._feat_cache is cache and d._grad_arena is arena and torch.equal(arena, snap)
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    assert all(q.grad is None for q in d.parameters()) and not ld.requires_grad
    _, lb = p.perturbation_test(m, x, mp, target=1, fractions=FRACTIONS, return_logits=True)
    assert torch.equal(ld, lb)                                                    # the evaluation logits of the same parameters


# ------------------------------------------------------------------------------------------------ 5. end to end, Fus_CrossViT
@pytest.fixture(scope="module")
def pair():
    import vits_returnftrs as vits
    fus = importlib.import_module(FUS_MOD)
    backs = []
    for i in range(2):
        b = vits.vit_small(num_classes=3, depth=2)
        b.load_state_dict(ref_vit.seeded_params(17 + i, num_classes=3, depth=2))
        backs.append(b.to(DEV))
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(ref_fusion.seeded_fusion_params(19))
    B = 2
    return model.to(DEV), backs, rng_tensor(93, (B, 3, 224, 224)), rng_tensor(94, (B, 3, 224, 224)), rng_tensor(95, (B, 14, 14))


def _fus_forward(model, backs, xc, xe):
    mods = [model] + backs
    was = [m.training for m in mods]
    for m in mods:
        m.eval()
    try:
        with torch.no_grad():
            fused, x_c, x_e = model(backs[0], backs[1], xc.to(DEV), xe.to(DEV))
            return fused + x_c + x_e
    finally:
        for m, w in zip(mods, was):
            m.train(w)


@pytest.mark.gpu
def test_fus_crossvit_logits_are_the_models_on_the_reference_masks(pair):
    p = _p()
    model, backs, xc, xe, mp = pair
    B, P = 2, 196
    target = torch.tensor([1, 2])
    fill = ([0.1, -0.2, 0.3], None)                                               # each stream its own fill
    args = (backs[0], backs[1], xc.to(DEV), xe.to(DEV))
    meter, both = model.perturbation_test(*args, maps=(mp.to(DEV), mp.to(DEV)), target=target, fractions=FRACTIONS, fill=fill, return_logits=True)
    _, only = model.perturbation_test(*args, maps=(mp.to(DEV), None), target=target, fractions=FRACTIONS, fill=fill, return_logits=True)
    assert both.shape == only.shape == (4, B, 3)
    rank = p.patch_rank(mp.to(DEV)).cpu().numpy()
    ranges = p.ranges_for(P, p.step_counts(P, FRACTIONS), "positive").tolist()
    mc = R.ref_perturb(xc.numpy(), rank, ranges, np.array(fill[0], np.float32))
    me = R.ref_perturb(xe.numpy(), rank, ranges, np.zeros(3, np.float32))
    for s in range(4):
        assert torch.equal(both[s], _fus_forward(model, backs, torch.from_numpy(mc[s]), torch.from_numpy(me[s]))), f"step {s}"
        # one map None: the enhanced batch of every step is the input itself
        assert torch.equal(only[s], _fus_forward(model, backs, torch.from_numpy(mc[s]), xe)), f"step {s}, cxr only"
    assert torch.equal(both[0], only[0]) and not torch.equal(both[3], only[3])     # the stream-ablation curve differs at fraction 1
    c, n, s = (v.cpu() for v in meter._views())
    _assert_score((c, s, n), R.ref_score(both.cpu().numpy(), target.numpy()), "fus")
    # target None: the argmax of step 0 of the summed output
    a = model.perturbation_test(*args, maps=(None, mp.to(DEV)), fractions=FRACTIONS)
    b = model.perturbation_test(*args, maps=(None, mp.to(DEV)), target=_fus_forward(model, backs, xc, xe).argmax(dim=1), fractions=FRACTIONS)
    assert torch.equal(a._buf, b._buf)
    assert model.training and all(v.training for v in backs)
    assert all(q.grad is None for v in backs for q in v.parameters()) and all(q.grad is None for q in model.parameters())


@pytest.mark.gpu
def test_fus_crossvit_refuses_wrong_encoders(pair):
    model, backs, xc, xe, mp = pair
    other = _encoder(seed=3)
    with pytest.raises(ValueError):
        model.perturbation_test(backs[0], other, xc.to(DEV), xe.to(DEV), maps=(mp.to(DEV), None))
    with pytest.raises(ValueError):
        model.perturbation_test(backs[1], backs[0], xc.to(DEV), xe.to(DEV), maps=(mp.to(DEV), None))
    with pytest.raises(ValueError):
        model.perturbation_test(backs[0], backs[1], xc.to(DEV), xe[:1].to(DEV), maps=(mp.to(DEV), None))
