"""CPU: the CKA reference is pinned against independent forms of the same definitions, its gates pass an honest f32 emulation and catch
the mutations a Gram / HSIC kernel can suffer, and the library's host-only entries (plan, work size, hidden-state layout, argument
domain) answer without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import cka_ref


def gauss(seed, shape):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)


# ---------------------------------------------------------------------------------------------------- the reference, pinned
@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_hsic1_formula_equals_the_u_statistic(n):
    K, L = cka_ref.gram_centered(gauss(10 + n, (n, 9))), cka_ref.gram_centered(gauss(20 + n, (n, 5)))
    assert abs(cka_ref.hsic1(K, L) - cka_ref.hsic1_ustat(K, L)) <= 5e-12
    assert abs(cka_ref.hsic1(K, K) - cka_ref.hsic1_ustat(K, K)) <= 5e-12


def test_hsic0_from_the_three_sums_equals_the_trace():
    K, L = cka_ref.gram_centered(gauss(31, (9, 12))), cka_ref.gram_centered(gauss(32, (9, 7)))
    assert abs(cka_ref.hsic0(K, L) - cka_ref.hsic0_trace(K, L)) <= 1e-12 * abs(cka_ref.hsic0_trace(K, L))
    # and on Gram matrices that are NOT centred (the kernel's shift is its own f32 mean)
    x, y = gauss(33, (9, 12)) + 3.0, gauss(34, (9, 7)) - 2.0
    assert abs(cka_ref.hsic0(x @ x.T, y @ y.T) - cka_ref.hsic0_trace(K := cka_ref.gram_centered(x), cka_ref.gram_centered(y))) <= 1e-10 * abs(cka_ref.hsic0(K, K))


@pytest.mark.parametrize("unbiased", [True, False])
def test_hsic_is_invariant_to_a_column_shift(unbiased):
    x, y = gauss(41, (11, 20)) + 5.0, gauss(42, (11, 13))
    ref = cka_ref.hsic(cka_ref.gram_centered(x), cka_ref.gram_centered(y), unbiased)
    for sx in (0.0, x.mean(axis=0, keepdims=True), 3.25, gauss(43, (1, 20))):
        xs = x - sx
        got = cka_ref.hsic(xs @ xs.T, cka_ref.gram_centered(y), unbiased)
        assert abs(got - ref) <= 2e-12


def test_gram_form_of_biased_cka_equals_the_feature_space_form():
    x, y = gauss(51, (16, 30)), gauss(52, (16, 12))
    assert abs(cka_ref.cka(x, y, unbiased=False) - cka_ref.cka_feature_space(x, y)) <= 3e-16


@pytest.mark.parametrize("unbiased", [True, False])
def test_cka_identities(unbiased):
    x = gauss(61, (12, 10))
    assert abs(cka_ref.cka(x, x, unbiased) - 1.0) <= 1e-14
    q, _ = np.linalg.qr(gauss(62, (10, 10)))
    y = gauss(63, (12, 6))
    ref = cka_ref.cka(x, y, unbiased)
    assert abs(cka_ref.cka(x @ q, y, unbiased) - ref) <= 1e-13
    assert abs(cka_ref.cka(3.7 * x, 0.2 * y, unbiased) - ref) <= 1e-13
    m = cka_ref.cka_matrix([np.stack([x, x @ q])], [np.stack([x, 2 * x, x @ q])], unbiased)
    assert m.shape == (2, 3) and np.abs(m - 1.0).max() <= 1e-13


def test_minibatch_cka_sums_hsic_before_the_ratio():
    xs, ys = [gauss(70 + i, (n, 8)) for i, n in enumerate((5, 9, 6))], [gauss(80 + i, (n, 4)) for i, n in enumerate((5, 9, 6))]
    Ks, Ls = [cka_ref.gram_centered(x) for x in xs], [cka_ref.gram_centered(y) for y in ys]
    want = sum(cka_ref.hsic1(K, L) for K, L in zip(Ks, Ls)) / np.sqrt(sum(cka_ref.hsic1(K, K) for K in Ks) * sum(cka_ref.hsic1(L, L) for L in Ls))
    assert cka_ref.cka_from_grams(Ks, Ls) == want
    assert cka_ref.cka_matrix([x[None] for x in xs], [y[None] for y in ys])[0, 0] == want


# ---------------------------------------------------------------------------------------------------- the gates
def dc_err(g, x):
    return np.abs(cka_ref.double_center(g) - cka_ref.double_center(cka_ref.gram_centered(x)))


@pytest.mark.parametrize("n,k", [(5, 130), (33, 700), (64, 1920)])
def test_an_honest_f32_gram_sits_inside_the_gate(n, k):
    x = cka_ref.offset_gaussians(n, k, 90 + n)
    err, gate = dc_err(cka_ref.gram_f32_emulated(x), x), cka_ref.gram_gate(x)
    assert (err <= gate).all(), float((err / gate).max())
    assert (err / gate).max() > 1e-4          # (the gate is not vacuous: the emulation's error is within 4 orders of it)


@pytest.mark.parametrize("n,k", [(4, 65), (5, 257), (33, 300)])
def test_f32_emulation_is_exact_on_exact_inputs(n, k):
    x = cka_ref.exact_inputs(n, k, 100 + n)
    assert (x.sum(axis=0) == 0).all() and np.abs(x).max() <= 4
    assert np.array_equal(cka_ref.gram_f32_emulated(x), (x @ x.T).astype(np.float64))
    assert np.array_equal(cka_ref.gram_centered(x), (x @ x.T).astype(np.float64))


def test_gram_gate_catches_a_dropped_last_stage_and_an_unmasked_pad_row():
    n, k, stage = 33, 300, 64
    x = cka_ref.offset_gaussians(n, k, 111)
    gate = cka_ref.gram_gate(x)
    dropped = cka_ref.gram_f32_emulated(x[:, :k - k % stage])                    # the last (partial) column stage never multiplied
    assert (dc_err(dropped, x) > gate).any()
    # A pad row (zero-filled, then centred like a real one: it holds -m) is harmless INSIDE the n x n block as long as it only shifts every row
    # alike - entering the column mean, or adding the constant m'm to every element: both estimators and H g H are invariant to that by
    # construction, and the gate rightly lets it pass.  What it must catch is the pad row reaching the SUMS: row / column n multiplied and reduced
    # as if it were an example (the block's last row overwritten by the pad row's products).
    m = x.astype(np.float64).mean(axis=0)
    K = cka_ref.gram_centered(x)
    assert (dc_err(K + m @ m, x) <= gate).all()
    xp = np.concatenate([x, np.zeros((1, k), np.float32)]).astype(np.float64)
    shifted_mean = (xp - xp.mean(axis=0)) @ (xp - xp.mean(axis=0)).T
    assert (dc_err(shifted_mean[:n, :n], x) <= gate).all()
    leaked = K.copy()
    leaked[n - 1, :] = leaked[:, n - 1] = (x.astype(np.float64) - m) @ (-m)       # the last example's products replaced by the pad row's
    leaked[n - 1, n - 1] = m @ m
    assert (dc_err(leaked, x) > gate).any()
    assert abs(cka_ref.hsic1(leaked, leaked) - cka_ref.hsic1(K, K)) > cka_ref.hsic_gate(K, K)


def test_hsic_gate_catches_a_diagonal_left_in():
    x, y = cka_ref.offset_gaussians(33, 200, 121), cka_ref.offset_gaussians(33, 90, 122)
    K, L = cka_ref.gram_centered(x), cka_ref.gram_centered(y)
    with_diag = cka_ref._sums(K, L, False)
    c2, c3, den = cka_ref._coef(33, True)
    mutant = (with_diag[0] + c2 * with_diag[1] - c3 * with_diag[2]) / den     # the unbiased coefficients on sums that kept the diagonals
    assert abs(mutant - cka_ref.hsic1(K, L)) > cka_ref.hsic_gate(K, L)
    # reordering the sums stays inside: rows reversed
    assert abs(cka_ref.hsic1(K[::-1, ::-1], L[::-1, ::-1]) - cka_ref.hsic1(K, L)) <= cka_ref.hsic_gate(K, L)


# ---------------------------------------------------------------------------------------------------- the library, without a GPU
NEW = {"mfvit_gram_plan": 3, "mfvit_gram_work_bytes": 3, "mfvit_gram_centered": 10, "mfvit_hsic_accumulate": 10, "mfvit_vit_hidden_layout": 2}


def test_new_symbols_are_exported_and_bound():
    from mfvit import _lib
    h = _lib.lib()
    for name, arity in NEW.items():
        assert hasattr(h, name), name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    assert h.mfvit_abi_version() == 5 and _lib.ABI_VERSION == 5


def plan_of(n, k):
    from mfvit import _lib
    p = (ctypes.c_int32 * 4)()
    assert _lib.lib().mfvit_gram_plan(n, k, p) == 0
    return list(p)


@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 255, 256, 257, 384, 1920, 75264, 75648, 151296, 10 ** 7])
def test_gram_plan_is_self_consistent(k):
    stage, splits, cps, last = plan_of(64, k)
    assert stage >= 1 and splits >= 1 and cps % stage == 0 and 1 <= last <= cps
    assert (splits - 1) * cps + last == k
    assert plan_of(2, k) == plan_of(256, k) == [stage, splits, cps, last]        # (today: a function of k alone)
    from mfvit import _lib
    h = _lib.lib()
    for n in (2, 33, 256):
        nt = (n + 31) // 32
        assert h.mfvit_gram_work_bytes(1, n, k) >= splits * (nt * (nt + 1) // 2) * 1024 * 4
        assert h.mfvit_gram_work_bytes(13, n, k) == 13 * h.mfvit_gram_work_bytes(1, n, k)


def test_gram_plan_has_the_edges_the_gpu_test_asks_for():
    stage, _, cps, _ = plan_of(64, 1)
    assert plan_of(64, cps)[1] == 1 and plan_of(64, cps + 1)[1:] == [2, cps, 1]  # one split exactly; a last split of exactly one column
    assert plan_of(64, stage)[3] == stage


def test_einval_domain():
    from mfvit import _lib
    h = _lib.lib()
    E = -22
    p = (ctypes.c_int32 * 4)()
    for n, k in ((1, 8), (257, 8), (0, 8), (-3, 8), (8, 0), (8, -1)):
        assert h.mfvit_gram_plan(n, k, p) == E
        assert h.mfvit_gram_work_bytes(1, n, k) == 0
    assert h.mfvit_gram_plan(8, 8, None) == E
    assert h.mfvit_gram_work_bytes(0, 8, 8) == 0 and h.mfvit_gram_work_bytes(65, 8, 8) == 0 and h.mfvit_gram_work_bytes(64, 8, 8) > 0
    # (host addresses that are never dereferenced: every call below is refused before any HIP call)
    buf = (ctypes.c_double * 64)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    wb = h.mfvit_gram_work_bytes(2, 8, 16)
    ok = dict(x=a, rep_stride=256, ld=16, reps=2, n=8, k=16, g=a, work=a, wb=wb)

    def gram(**kw):
        c = dict(ok, **kw)
        return h.mfvit_gram_centered(c["x"], c["rep_stride"], c["ld"], c["reps"], c["n"], c["k"], c["g"], c["work"], c["wb"], None)
    for bad in (dict(x=None), dict(g=None), dict(work=None), dict(reps=0), dict(reps=65), dict(n=1), dict(n=257), dict(k=0), dict(ld=12), dict(ld=18),
                dict(rep_stride=130), dict(x=a + 4), dict(x=a + 8), dict(wb=wb - 1), dict(wb=0), dict(k=17, ld=16)):
        assert gram(**bad) == E, bad

    def hs(ga=a, ra=2, gb=a, rb=3, n=8, unbiased=1, ab=a, aa=a, bb=a):
        return h.mfvit_hsic_accumulate(ga, ra, gb, rb, n, unbiased, ab, aa, bb, None)
    for bad in (dict(ga=None), dict(gb=None), dict(ab=None), dict(aa=None), dict(bb=None), dict(ra=0), dict(ra=65), dict(rb=0), dict(rb=65), dict(n=3),
                dict(n=257), dict(n=1, unbiased=0), dict(n=0, unbiased=0)):
        assert hs(**bad) == E, bad


@pytest.mark.parametrize("arch,img,depth,B", [("vit_small", 224, 12, 2), ("vit_small", 32, 3, 4), ("vit_base", 224, 2, 3)])
def test_hidden_layout_lies_inside_the_workspace(arch, img, depth, B):
    import vits
    from mfvit import _lib
    h = _lib.lib()
    m = getattr(vits, arch)(num_classes=3, depth=depth, img_size=img)
    cfg = m._cfg(torch.zeros(B, 3, img, img), True)
    out = (ctypes.c_int64 * 2)()
    assert h.mfvit_vit_hidden_layout(cfg, out) == 0
    state = B * m.num_tokens * m.embed_dim * 4
    assert out[0] >= 0 and out[0] % 16 == 0 and out[1] % 16 == 0 and out[1] >= state
    assert out[0] + depth * out[1] + state <= h.mfvit_vit_workspace_bytes(cfg)
    assert h.mfvit_vit_hidden_layout(m._cfg(torch.zeros(B, 3, img, img), False), out) == -22      # nothing is kept without save_for_backward
    assert h.mfvit_vit_hidden_layout(cfg, None) == -22
    assert h.mfvit_vit_hidden_layout(m._cfg(torch.zeros(B, 3, img, img - 4), True), out) == -22


def test_python_surface():
    import vits
    from mfvit import similarity
    m = vits.vit_small(num_classes=3, depth=2)
    for name in ("hidden_states", "get_intermediate_layers"):
        assert callable(getattr(m, name))
    assert similarity.MAX_N == 256
    with pytest.raises(ValueError, match="mean pooling"):
        similarity.layerwise([m, m], [], [(0, 1)], tokens="mean")
    with pytest.raises(ValueError, match="drop_last"):
        list(similarity._minibatches([torch.zeros(259, 1)], True))
    assert [x[0].shape[0] for x in similarity._minibatches([torch.zeros(600, 1)], True)] == [256, 256, 88]
    with pytest.raises(ValueError):
        m.get_intermediate_layers(torch.zeros(1, 3, 224, 224), n=[5])
    with pytest.raises(ValueError):
        m.get_intermediate_layers(torch.zeros(1, 3, 224, 224), n=3)
