"""GPU: bootstrap replicates and DeLong components (csrc/evalstats.hip) through the C ABI and through mfvit.evalstats, every integer bit for bit
against tests/evalstats_ref.py, at the sizes where the kernels' loops turn over: the 256-sample block of the order kernel, its 1,024-key LDS
chunk and the 512-place tile of the prefix scan, each minus one, exact and plus one."""
import numpy as np
import pytest
import torch

import evalstats_ref as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_EDGES = (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
KINDS = ("gauss", "ties", "equal", "special")
LKINDS = ("random", "outside", "missing")
EXTRA, PADROWS = 3, 2                      # NaN columns beside the C scores and NaN rows between the models: ld = C + 3, a padded model stride
SENTINEL = -0x0123456789ABCDEF             # what every output word holds before a call (outputs are overwritten) and what the guard words keep
GUARD = 8


def _guarded(numel, dtype=torch.int64):
    fill = SENTINEL if dtype == torch.int64 else -0x01234567
    buf = torch.full((GUARD + numel + GUARD,), fill, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + numel], fill


def _intact(g):
    buf, _, fill = g
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _layout(scores):
    """scores [M, n, C] as the slice wide[:, :n, :C] of a NaN-filled [M, n + PADROWS, C + EXTRA] tensor"""
    M, n, C = scores.shape
    wide = torch.full((M, n + PADROWS, C + EXTRA), float("nan"), device=DEV)
    wide[:, :n, :C] = torch.from_numpy(scores).to(DEV)
    view = wide[:, :n, :C]
    assert view.stride(1) == C + EXTRA and view.stride(0) == (n + PADROWS) * (C + EXTRA) and view.data_ptr() == wide.data_ptr()
    return wide, view


def _work(nbytes):
    """a scratch buffer full of 0xA5 (its contents mean nothing to a call) with guard bytes behind it"""
    buf = torch.full((nbytes + 256,), 0xA5, device=DEV, dtype=torch.uint8)
    return buf


def _boot(scores, labels, seed, r0, R, stratified, want_conf=True, want_auc=True):
    """One mfvit_boot_counts call -> (conf [R, M, C, C], u2 [R, M, C], npos [R, C]) as int64 numpy arrays (SENTINEL where not asked for)"""
    from mfvit._lib import check, lib, ptr, stream
    M, n, C = scores.shape
    wide, view = _layout(scores)
    lab = torch.from_numpy(labels).to(DEV)
    wide0, lab0 = wide.clone(), lab.clone()
    conf, u2, npos = _guarded(R * M * C * C), _guarded(R * M * C), _guarded(R * C)
    nbytes = lib().mfvit_boot_work_bytes(n, C, M, R)
    assert nbytes > 0
    work = _work(nbytes)
    check(lib().mfvit_boot_counts(ptr(view), view.stride(1), view.stride(0), ptr(lab), n, C, M, seed, r0, R, int(stratified), ptr(work), nbytes,
                                  ptr(conf[1]) if want_conf else None, ptr(u2[1]) if want_auc else None, ptr(npos[1]) if want_auc else None, stream()),
          "mfvit_boot_counts")
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int32), wide0.view(torch.int32)) and torch.equal(lab, lab0)          # inputs are read-only
    assert _intact(conf) and _intact(u2) and _intact(npos) and bool((work[nbytes:] == 0xA5).all())
    return conf[1].view(R, M, C, C).cpu().numpy(), u2[1].view(R, M, C).cpu().numpy(), npos[1].view(R, C).cpu().numpy()


def _delong(scores, labels, want_v2=True):
    from mfvit._lib import check, lib, ptr, stream
    M, n, C = scores.shape
    wide, view = _layout(scores)
    lab = torch.from_numpy(labels).to(DEV)
    wide0 = wide.clone()
    v2, pxy, nxy, u2, npos = _guarded(M * C * n, torch.int32), _guarded(C * M * M), _guarded(C * M * M), _guarded(M * C), _guarded(C)
    nbytes = lib().mfvit_boot_work_bytes(n, C, M, 1)
    work = _work(nbytes)
    check(lib().mfvit_delong_counts(ptr(view), view.stride(1), view.stride(0), ptr(lab), n, C, M, ptr(work), nbytes, ptr(v2[1]) if want_v2 else None,
                                    ptr(pxy[1]), ptr(nxy[1]), ptr(u2[1]), ptr(npos[1]), stream()), "mfvit_delong_counts")
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int32), wide0.view(torch.int32))
    assert all(_intact(g) for g in (v2, pxy, nxy, u2, npos)) and bool((work[nbytes:] == 0xA5).all())
    return (v2[1].view(M, C, n).cpu().numpy(), pxy[1].view(C, M, M).cpu().numpy(), nxy[1].view(C, M, M).cpu().numpy(),
            u2[1].view(M, C).cpu().numpy(), npos[1].cpu().numpy())


def _same(got, want, what):
    for g, w, name in zip(got, want, ("conf", "u2", "npos")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


# ------------------------------------------------------------------------------------------------------- mfvit_boot_counts
@pytest.mark.parametrize("n", N_EDGES)
def test_boot_counts_bit_exact_at_block_chunk_and_tile_edges(n):
    i = N_EDGES.index(n)
    M, C, R = (1, 3)[i % 2], 3, 4
    for k, kind in enumerate(KINDS):
        lkind = LKINDS[(i + k) % 3]
        strat = (i + k) % 2 == 1
        s, t = E.case(n, C, M, kind, lkind, 31 * n + k)
        want = E.boot_counts(s, t, seed=1000 + n, r0=0, R=R, stratified=strat, brute=n <= 300)
        _same(_boot(s, t, 1000 + n, 0, R, strat), want, (n, kind, lkind, strat))


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 3, 64])
def test_boot_counts_class_and_model_counts(C, M):
    n, R = 300, 3
    for kind, lkind, strat in (("special", "outside", True), ("ties", "missing", False)):
        s, t = E.case(n, C, M, kind, lkind, 100 * C + M)
        want = E.boot_counts(s, t, seed=C, r0=0, R=R, stratified=strat, brute=C <= 3)
        _same(_boot(s, t, C, 0, R, strat), want, (C, M, kind, lkind))


def test_boot_counts_at_the_largest_sample_count():
    """n = 32768: the scan's prefix takes 128 KiB of LDS, a histogram counter may reach 2^15; against the sort-based reference"""
    n, C = 32768, 2
    s, t = E.case(n, C, 1, "ties", "random", 99)
    s[0, 100:140, 0] = np.nan
    for strat in (False, True):
        want = E.boot_counts(s, t, seed=(7 << 32) + 5, r0=0, R=2, stratified=strat, brute=False)
        _same(_boot(s, t, (7 << 32) + 5, 0, 2, strat), want, ("n = 32768", strat))


def test_boot_counts_replicates_are_absolute_and_calls_repeat_their_bits():
    n, C, M = 700, 3, 3
    s, t = E.case(n, C, M, "ties", "outside", 4)
    seed = 0xFEDCBA9876543210
    for strat in (False, True):
        whole = _boot(s, t, seed, 0, 7, strat)
        _same(whole, E.boot_counts(s, t, seed=seed, r0=0, R=7, stratified=strat, brute=False), "one call")
        _same(_boot(s, t, seed, 0, 7, strat), whole, "the same call again")
        parts = [_boot(s, t, seed, r0, R, strat) for r0, R in ((0, 2), (2, 4), (6, 1))]
        _same([np.concatenate([p[k] for p in parts]) for k in range(3)], whole, "chunks")
    late = _boot(s, t, seed, 123456, 3, False)
    _same(late, E.boot_counts(s, t, seed=seed, r0=123456, R=3, brute=False), "r0 = 123456")


def test_boot_counts_past_the_replicates_of_one_launch():
    """the library launches 65,536 replicates at a time: replicates 65,534 .. 65,539 of one call lie on both sides of that turn-over"""
    n, C, M, R = 9, 2, 2, 65540
    s, t = E.case(n, C, M, "ties", "random", 3)
    for strat in (False, True):
        conf, u2, npos = _boot(s, t, 11, 0, R, strat)
        for r0, k in ((0, 3), (65534, 6)):
            want = E.boot_counts(s, t, seed=11, r0=r0, R=k, stratified=strat)
            _same((conf[r0:r0 + k], u2[r0:r0 + k], npos[r0:r0 + k]), want, (r0, strat))
        assert (npos.sum(1) == n).all() and (conf.sum((2, 3)) == n).all()          # every label is a class: each replicate holds n draws


def test_boot_counts_either_half_null():
    n, C, M, R = 400, 3, 2, 5
    s, t = E.case(n, C, M, "special", "outside", 6)
    for strat in (False, True):
        want = E.boot_counts(s, t, seed=2, r0=1, R=R, stratified=strat, brute=False)
        conf, u2, npos = _boot(s, t, 2, 1, R, strat, want_conf=False)
        assert (conf == SENTINEL).all()
        np.testing.assert_array_equal(u2, want[1])
        np.testing.assert_array_equal(npos, want[2])
        conf, u2, npos = _boot(s, t, 2, 1, R, strat, want_auc=False)
        np.testing.assert_array_equal(conf, want[0])
        assert (u2 == SENTINEL).all() and (npos == SENTINEL).all()


def test_replicate_zero_is_eval_counts_bit_for_bit():
    from mfvit import metrics
    n, C = 900, 3
    s, t = E.case(n, C, 1, "special", "outside", 13)
    conf, u2, npos = _boot(s, t, 5, 0, 1, False)
    econf, _, eu2, enpos = metrics.eval_counts(torch.from_numpy(s[0]).to(DEV), torch.from_numpy(t).to(DEV))
    np.testing.assert_array_equal(conf[0, 0], econf.cpu().numpy())
    np.testing.assert_array_equal(u2[0, 0], eu2.cpu().numpy())
    np.testing.assert_array_equal(npos[0], enpos.cpu().numpy())
    _, _, _, du2, dnpos = _delong(s, t)
    np.testing.assert_array_equal(du2[0], eu2.cpu().numpy())
    np.testing.assert_array_equal(dnpos, enpos.cpu().numpy())


# ------------------------------------------------------------------------------------------------------- mfvit_delong_counts
@pytest.mark.parametrize("n", N_EDGES)
def test_delong_counts_bit_exact_at_block_chunk_and_tile_edges(n):
    i = N_EDGES.index(n)
    M, C = (3, 1)[i % 2], 3
    for k, kind in enumerate(KINDS):
        lkind = LKINDS[(i + k) % 3]
        s, t = E.case(n, C, M, kind, lkind, 17 * n + k)
        want = E.delong_counts(s, t, brute=n <= 300)
        got = _delong(s, t)
        for g, w, name in zip(got, want, ("v2", "pos_xy", "neg_xy", "u2", "npos")):
            np.testing.assert_array_equal(g, w, err_msg=f"{name} {(n, kind, lkind)}")
        assert got[1].dtype == np.int64 and (got[1] == got[1].transpose(0, 2, 1)).all()          # the upper triangle mirrored


def test_delong_counts_class_counts_optional_v2_and_the_largest_sample_count():
    for n, C, M in ((300, 1, 2), (300, 2, 1), (300, 64, 3), (32768, 2, 1)):
        s, t = E.case(n, C, M, "ties", "outside" if C > 1 else "random", n + C)
        want = E.delong_counts(s, t, brute=False)
        got = _delong(s, t, want_v2=False)
        assert (got[0] == -0x01234567).all()
        for g, w, name in zip(got[1:], want[1:], ("pos_xy", "neg_xy", "u2", "npos")):
            np.testing.assert_array_equal(g, w, err_msg=f"{name} {(n, C, M)}")
        again = _delong(s, t)
        np.testing.assert_array_equal(again[0], want[0])
        for g, w in zip(again[1:], got[1:]):
            np.testing.assert_array_equal(g, w)


# ------------------------------------------------------------------------------------------------------- the Python layer
def _three_streams(n, C, seed):
    """Fus_CrossViT-shaped scores: three logit sets per sample (fused, cxr, enh); the meter sees their sum and the two single streams"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = rng.choice(C, size=n, p=[0.6, 0.3, 0.1]).astype(np.int64)
    fus, cxr, enh = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(3))
    for k, x in enumerate((fus, cxr, enh)):
        x[np.arange(n), t] += 0.5 + 0.25 * k
    return fus, cxr, enh, t


def _check_ci(res, names, want, what):
    models, pairs = want
    for m, nm in enumerate(names):
        for k, (point, lo, hi, dropped) in models[m].items():
            got = res.models[nm][k]
            np.testing.assert_allclose(np.ravel(got.point), point, rtol=0, atol=1e-12, equal_nan=True, err_msg=f"{what} {nm} {k}")
            np.testing.assert_allclose(np.ravel(got.lo), lo, rtol=0, atol=1e-12, equal_nan=True, err_msg=f"{what} {nm} {k}")
            np.testing.assert_allclose(np.ravel(got.hi), hi, rtol=0, atol=1e-12, equal_nan=True, err_msg=f"{what} {nm} {k}")
            assert np.ravel(got.dropped).tolist() == dropped
    for (a, b), stats in pairs.items():
        for k, (point, lo, hi, p, used) in stats.items():
            got = res.pairs[(names[a], names[b])][k]
            for g, w in ((got.point, point), (got.lo, lo), (got.hi, hi), (got.p, p)):
                np.testing.assert_allclose(np.ravel(g), w, rtol=0, atol=1e-12, equal_nan=True, err_msg=f"{what} {a} {b} {k}")
            assert np.ravel(got.used).tolist() == used


def _check_delong(res, want, what):
    for k, v in (("auc", res.auc), ("var", res.var), ("lo", res.lo), ("hi", res.hi), ("cov", res.cov), ("z", res.z), ("p", res.p)):
        np.testing.assert_allclose(v, want[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=f"{what} {k}")


def test_paired_meter_over_ragged_batches_of_a_two_stream_model():
    from mfvit import evalstats
    n, C, n_boot = 700, 3, 40
    fus, cxr, enh, t = _three_streams(n, C, 21)
    names = ["sum", "cxr", "enh"]
    meter = evalstats.PairedMeter(names, C)
    i = 0
    for bs in (256, 1, 255, 188):
        f, c, e = (torch.from_numpy(x[i:i + bs]).to(DEV) for x in (fus, cxr, enh))
        meter.update({"sum": f + c + e, "cxr": c, "enh": e}, torch.from_numpy(t[i:i + bs]).to(DEV).float())      # labels arrive as floats
        i += bs
    assert i == n
    scores = np.stack([(torch.from_numpy(fus) + torch.from_numpy(cxr) + torch.from_numpy(enh)).numpy(), cxr, enh])
    for strat in (False, True):
        res = meter.bootstrap_ci(n_boot=n_boot, level=0.9, seed=77, stratified=strat)
        assert res.names == names and res.n_boot == n_boot
        _check_ci(res, names, E.bootstrap_ci_ref(scores, t, n_boot, 0.9, 77, strat), f"stratified={strat}")
    dl = meter.delong(level=0.9)
    _, pos_xy, neg_xy, u2, npos = E.delong_counts(scores, t, brute=False)
    _check_delong(dl, E.delong_from_counts(pos_xy, neg_xy, u2, npos, n, 0.9), "PairedMeter.delong")
    assert dl.names == names and np.isfinite(dl.p[0, 0, 1])


def test_bootstrap_counts_chunks_and_epoch_meter_delegates():
    from mfvit import evalstats, metrics
    n, C = 500, 3
    _, cxr, _, t = _three_streams(n, C, 8)
    sd, td = torch.from_numpy(cxr).to(DEV), torch.from_numpy(t).to(DEV)
    whole = evalstats.bootstrap_counts(sd, td, 10, seed=3)
    want = E.boot_counts(cxr, t, seed=3, r0=0, R=11, brute=False)
    for chunk in (1, 4, 11, 1000):
        got = evalstats.bootstrap_counts(sd, td, 10, seed=3, chunk=chunk)
        for g, w, x in zip(got, whole, want):
            assert torch.equal(g, w)
            np.testing.assert_array_equal(g.cpu().numpy(), x)
    meter = metrics.EpochMeter(C)
    meter.update(sd[:300], td[:300].float(), torch.zeros((), device=DEV))
    meter.update(sd[300:], td[300:].float(), torch.zeros((), device=DEV))
    res = meter.bootstrap_ci(n_boot=30, level=0.95, seed=1)
    _check_ci(res, ["0"], E.bootstrap_ci_ref(cxr, t, 30, 0.95, 1), "EpochMeter.bootstrap_ci")
    _, pos_xy, neg_xy, u2, npos = E.delong_counts(cxr, t, brute=False)
    _check_delong(meter.delong(), E.delong_from_counts(pos_xy, neg_xy, u2, npos, n), "EpochMeter.delong")
    _, auc, acc = meter.compute()                                         # the existing epoch numbers are the bootstrap's points
    assert abs(res.models["0"]["macro_auc"].point - auc) < 1e-12 and abs(res.models["0"]["accuracy"].point - acc) < 1e-12
