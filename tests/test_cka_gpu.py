"""GPU: the centred Gram and HSIC kernels (csrc/cka.hip) against tests/cka_ref.py, the encoder's hidden states against the CPU oracle, and
minibatch CKA end to end (mfvit/similarity.py, Fus_CrossViT.stream_similarity).  The gates are cka_ref's (derived there); the end-to-end gate
is the one profiles/cka_parity.txt records."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import cka_ref
from conftest import rng_tensor
from oracle import ref_vit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT = os.environ.get("MFVIT_PARITY_REPORT")      # a file the measured figures are appended to (they are printed either way: run with -s)
N_EDGES = [2, 4, 5, 31, 32, 33, 64, 65, 255, 256]
T, D = 197, 384
GUARD = 64
# End to end, the largest |CKA - reference| measured on an MI355X over this file's two seeds (profiles/cka_parity.txt): 9.32e-07 - the unbiased
# estimator at n = 8 (it drops the Gram's diagonal, so the f32 error of the off-diagonal sums of k = 75,648 products is all that is left to set
# against a small HSIC); the biased estimator on the same Gram matrices stays below 4e-10.  The error is a random walk over the inputs: gated at
# 4 x the measured value.  A measured error above 1e-5 would be a defect to explain, not a tolerance to widen.
E2E_MEASURED = 9.33e-7
E2E_GATE = 4 * E2E_MEASURED
# The two small cases, gated the same way (4 x the largest error measured on an MI355X): CKAMeter / linear_cka on k = 300 and k = 37 features of 9 and
# 16 examples, and cka() over 256 + 4 examples of a depth-1 encoder at 32^2.
METER_MEASURED = 7.35e-8
CUT_MEASURED = 2.19e-7
METER_GATE, CUT_GATE = 4 * METER_MEASURED, 4 * CUT_MEASURED


def log(msg):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")
    print(msg)


def plan_of(n, k):
    from mfvit import _lib
    p = (ctypes.c_int32 * 4)()
    assert _lib.lib().mfvit_gram_plan(n, k, p) == 0
    return list(p)


def gram_call(buf, col0, k, n, reps, poison=True):
    """mfvit_gram_centered on the view [:, :n, col0:col0 + k] of a (reps, rows, ld) f32 buffer: the (reps, n, n) float64 result, taken from a NaN-filled
    output with a guard band on both sides that must come back untouched; the work buffer is NaN-filled too."""
    from mfvit import _lib
    h = _lib.lib()
    assert buf.dtype == torch.float32 and buf.is_contiguous() and buf.dim() == 3
    rows, ld = buf.shape[1], buf.shape[2]
    nbytes = h.mfvit_gram_work_bytes(reps, n, k)
    assert nbytes > 0
    work = torch.full((nbytes // 4,), float("nan"), device=DEV) if poison else torch.empty(nbytes // 4, device=DEV)
    out = torch.full((reps * n * n + 2 * GUARD,), float("nan"), device=DEV, dtype=torch.float64)
    rc = h.mfvit_gram_centered(buf.data_ptr() + 4 * col0, rows * ld, ld, reps, n, k, out.data_ptr() + 8 * GUARD, work.data_ptr(), nbytes,
                               _lib.stream())
    assert rc == 0
    assert torch.isnan(out[:GUARD]).all() and torch.isnan(out[-GUARD:]).all(), "guard band written"
    g = out[GUARD:-GUARD].view(reps, n, n)
    assert torch.equal(g.view(torch.int64), g.view(torch.int64).transpose(1, 2)), "g[i][j] and g[j][i] differ in their bits"
    return g


def nan_buffer(reps, n, k, x):
    """(reps, n, ld) buffer, NaN everywhere but [:, :, :k] = x (numpy (reps, n, k)); ld leaves 4 .. 7 NaN columns behind the view."""
    ld = (k + 3) // 4 * 4 + 4
    buf = torch.full((reps, n, ld), float("nan"), dtype=torch.float32)
    buf[:, :, :k] = torch.from_numpy(np.asarray(x, dtype=np.float32))
    return buf.to(DEV)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# ---------------------------------------------------------------------------------------------------- Gram, exact inputs
def edge_ks():
    stage, _, cps, _ = plan_of(64, 1)
    return [1, 2, 3, stage - 1, stage, stage + 1, cps - 1, cps, cps + 1]     # cps + 1: two splits, the last of exactly one column


@pytest.mark.parametrize("n", N_EDGES)
def test_gram_is_exact_on_exact_inputs(n):
    ks = edge_ks()
    assert plan_of(n, ks[-1])[1:] == [2, ks[-2], 1] and plan_of(n, ks[-2])[1] == 1
    for k in ks:
        x = np.stack([cka_ref.exact_inputs(n, k, 1000 * n + 13 * k + r) for r in range(13)])
        xf = x.astype(np.float64)                      # (the int64 Gram, through float64 products: every sum is an integer below 2^53)
        want = torch.from_numpy(xf @ xf.transpose(0, 2, 1)).long()
        buf = nan_buffer(13, n, k, x)
        g13 = gram_call(buf, 0, k, n, 13)
        assert torch.equal(g13.cpu(), want.double()), (n, k)
        assert bits_equal(gram_call(buf, 0, k, n, 13), g13), "two calls differ"
        for r in (0, 7, 12):      # a representation computed alone has the bits it has among 13
            assert bits_equal(gram_call(buf[r:r + 1].contiguous(), 0, k, n, 1)[0], g13[r]), (n, k, r)


@pytest.mark.parametrize("n", [5, 33, 256])
def test_gram_token_views_of_a_hidden_state(n):
    """The three views of a [n][197 * 384] buffer (all: the buffer; cls: k = D; patch: base + D, k = (T - 1) D), everything outside the view NaN."""
    x = cka_ref.exact_inputs(n, T * D, 77 + n).reshape(n, T, D)
    for name, col0, k, sel in (("all", 0, T * D, x), ("cls", 0, D, x[:, 0]), ("patch", D, (T - 1) * D, x[:, 1:])):
        sel = sel.reshape(n, -1)
        buf = torch.full((1, n, T * D), float("nan"), dtype=torch.float32)
        buf[0, :, col0:col0 + k] = torch.from_numpy(sel.astype(np.float32))
        g = gram_call(buf.to(DEV), col0, k, n, 1)
        sf = sel.astype(np.float64)
        assert torch.equal(g[0].cpu(), torch.from_numpy(sf @ sf.T).long().double()), name


def test_gram_nan_stays_in_its_representation():
    n, k = 33, 300
    x = np.stack([cka_ref.offset_gaussians(n, k, 300 + r) for r in range(5)])
    clean = gram_call(nan_buffer(5, n, k, x), 0, k, n, 5)
    x[3, 17, 299] = np.nan
    g = gram_call(nan_buffer(5, n, k, x), 0, k, n, 5)
    assert torch.isnan(g[3]).all()
    for r in (0, 1, 2, 4):
        assert bits_equal(g[r], clean[r])


# ---------------------------------------------------------------------------------------------------- Gram, Gaussian inputs
_gauss = {}


def gaussians():
    """(256, 75,648) Gaussians with a 10 : 1 common offset, drawn once; every case takes its first n rows and k columns."""
    if "x" not in _gauss:
        _gauss["x"] = cka_ref.offset_gaussians(256, T * D, 4242)
    return _gauss["x"]


@pytest.mark.parametrize("k", [1920, T * D])
@pytest.mark.parametrize("n", N_EDGES)
def test_gram_gaussian_inputs_inside_the_gate(n, k):
    x = np.ascontiguousarray(gaussians()[:n, :k])
    g = gram_call(nan_buffer(1, n, k, x[None]), 0, k, n, 1)[0].cpu().numpy()
    err = np.abs(cka_ref.double_center(g) - cka_ref.double_center(cka_ref.gram_centered(x)))
    gate = cka_ref.gram_gate(x)
    log(f"gram gaussian n={n} k={k}: max err / gate = {float((err / gate).max()):.3e}, max err {float(err.max()):.3e}")
    assert (err <= gate).all()


# ---------------------------------------------------------------------------------------------------- HSIC
def hsic_call(ga, gb, n, unbiased, acc=None):
    from mfvit import _lib
    ra, rb = ga.shape[0], gb.shape[0]
    if acc is None:
        acc = torch.zeros(ra * rb + ra + rb, device=DEV, dtype=torch.float64)
    p = acc.data_ptr()
    rc = _lib.lib().mfvit_hsic_accumulate(ga.data_ptr(), ra, gb.data_ptr(), rb, n, int(unbiased), p, p + 8 * ra * rb, p + 8 * (ra * rb + ra), _lib.stream())
    assert rc == 0
    return acc


def device_grams(reps, n, k, seed):
    x = np.stack([cka_ref.offset_gaussians(n, k, seed + r) for r in range(reps)])
    return gram_call(nan_buffer(reps, n, k, x), 0, k, n, reps).contiguous()


def check_hsic(acc, Ka, Kb, unbiased, what):
    ra, rb = len(Ka), len(Kb)
    got = acc.cpu().numpy()
    worst = 0.0
    for i in range(ra):
        for j in range(rb):
            ref, gate = cka_ref.hsic(Ka[i], Kb[j], unbiased), cka_ref.hsic_gate(Ka[i], Kb[j], unbiased)
            worst = max(worst, abs(got[i * rb + j] - ref) / gate)
    for o, Ks in ((ra * rb, Ka), (ra * rb + ra, Kb)):
        for i, K in enumerate(Ks):
            worst = max(worst, abs(got[o + i] - cka_ref.hsic(K, K, unbiased)) / cka_ref.hsic_gate(K, K, unbiased))
    log(f"hsic {what}: worst err / gate = {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("unbiased", [True, False])
@pytest.mark.parametrize("ra,rb", [(1, 1), (2, 3), (28, 28)])
@pytest.mark.parametrize("n", [4, 5, 33, 256])
def test_hsic_against_the_reference_on_the_device_gram(n, ra, rb, unbiased):
    ga, gb = device_grams(ra, n, 96, 500 + n), device_grams(rb, n, 40, 900 + n)
    acc = hsic_call(ga, gb, n, unbiased)
    check_hsic(acc, ga.cpu().numpy(), gb.cpu().numpy(), unbiased, f"n={n} {ra}x{rb} unbiased={unbiased}")
    assert bits_equal(hsic_call(ga, gb, n, unbiased), acc), "two runs differ"
    # gb == ga: the cross terms are the self terms
    same = hsic_call(ga, ga, n, unbiased).cpu().numpy()
    assert np.array_equal(same[:ra * ra].reshape(ra, ra).diagonal(), same[ra * ra:ra * ra + ra])
    assert np.array_equal(same[ra * ra:ra * ra + ra], same[ra * ra + ra:])
    check_hsic(torch.from_numpy(same), ga.cpu().numpy(), ga.cpu().numpy(), unbiased, f"n={n} {ra}x{ra} gb == ga unbiased={unbiased}")


@pytest.mark.parametrize("unbiased", [True, False])
def test_hsic_accumulates_over_minibatches_of_different_n(unbiased):
    ra, rb = 2, 3
    acc, refs = None, np.zeros(ra * rb + ra + rb)
    gates = np.zeros_like(refs)
    for n in (33, 5, 64):
        ga, gb = device_grams(ra, n, 96, 50 + n), device_grams(rb, n, 40, 60 + n)
        acc = hsic_call(ga, gb, n, unbiased, acc)
        Ka, Kb = ga.cpu().numpy(), gb.cpu().numpy()
        pairs = [(Ka[i], Kb[j]) for i in range(ra) for j in range(rb)] + [(K, K) for K in Ka] + [(K, K) for K in Kb]
        refs += [cka_ref.hsic(K, L, unbiased) for K, L in pairs]
        gates += [cka_ref.hsic_gate(K, L, unbiased) for K, L in pairs]
    err = np.abs(acc.cpu().numpy() - refs)
    assert (err <= gates + 4 * cka_ref.U53 * np.abs(refs)).all(), float((err / gates).max())


def test_meter_and_linear_cka_follow_the_reference():
    from mfvit import similarity
    xs = [torch.from_numpy(np.stack([cka_ref.offset_gaussians(n, 6 * 50, 700 + n + r) for r in range(3)])).to(DEV).view(3, n, 6, 50) for n in (9, 16)]
    ys = [torch.from_numpy(np.stack([cka_ref.offset_gaussians(n, 37, 800 + n + r) for r in range(2)])).to(DEV) for n in (9, 16)]      # (k % 4 != 0: the copy path)
    for unbiased in (True, False):
        m = similarity.CKAMeter(3, 2, unbiased)
        for x, y in zip(xs, ys):
            m.update(x, y)
        ref = cka_ref.cka_matrix([x.cpu().numpy() for x in xs], [y.cpu().numpy() for y in ys], unbiased)
        assert m.result().shape == (3, 2) and m.result().dtype == np.float64
        one = similarity.linear_cka(xs[1][0], ys[1][1], unbiased)
        errs = float(np.abs(m.result() - ref).max()), abs(one - cka_ref.cka(xs[1][0].cpu().numpy(), ys[1][1].cpu().numpy(), unbiased))
        log(f"meter / linear_cka unbiased={unbiased}: |CKA - ref| = {errs[0]:.3e} / {errs[1]:.3e} (gate {METER_GATE:.3e})")
        assert isinstance(one, float) and max(errs) <= METER_GATE
    assert abs(similarity.linear_cka(xs[0][0], xs[0][0]) - 1.0) <= 1e-12
    with pytest.raises(ValueError, match="drop_last"):
        similarity.CKAMeter(1, 1).update(xs[0][:1, :3], xs[0][:1, :3])
    with pytest.raises(_mfvit_error()):
        similarity.linear_cka(xs[0][0].cpu(), xs[0][0].cpu())


def _mfvit_error():
    from mfvit import MfvitError
    return MfvitError


# ---------------------------------------------------------------------------------------------------- hidden states
from test_encoder_gpu import build, scale_err  # noqa: E402  (the encoder tests' own model builder and error measure)

_oracle = {}


def oracle_states(img):
    """(params' seed 901, images' seed 902): oracle hidden states (4, 4, T, D) and features3D of depth 3, B = 4, computed once per image size."""
    if img not in _oracle:
        p = ref_vit.seeded_params(901, num_classes=3, depth=3, img_size=img)
        x = rng_tensor(902, (4, 3, img, img))
        with torch.no_grad():
            _oracle[img] = (x, cka_ref.oracle_hidden_states(p, x), ref_vit.features3d(p, x))
    return _oracle[img]


@pytest.mark.parametrize("img", [224, 32])
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16x3", 1e-3), ("bf16", 4e-2)])
def test_hidden_states_match_the_oracle(precision, tol, img):
    m, _ = build(precision, 901, depth=3, img=img)
    x, ref_h, ref_f = oracle_states(img)
    xg = x.to(DEV)
    m.train()
    f0 = m.features3D(xg)
    cache = m._feat_cache
    assert cache is not None
    h = m.hidden_states(xg)
    assert m._feat_cache is cache and m.training, "the feature cache / training flag moved"
    tokens = (img // 16) ** 2 + 1
    assert h.shape == (4, 4, tokens, 384) and h.dtype == torch.float32 and h.is_contiguous()
    for l in range(4):
        e = scale_err(h[l], ref_h[l])
        log(f"hidden_states[{precision}, {img}] layer {l}: {e:.2e}")
        assert e < tol, (l, e)
    # the last state through the final norm is features3D; so is get_intermediate_layers(n=1, norm=True) with its prefix token
    with torch.no_grad():
        normed = m._final_norm(h[-1])
    (patches, cls), = m.get_intermediate_layers(xg, n=1, norm=True, return_prefix_tokens=True)
    for got in (normed, torch.cat([cls, patches], dim=1)):
        assert scale_err(got, ref_f) < tol
        assert scale_err(got, f0) < tol
    assert m._feat_cache is cache and m.training
    m.eval()
    assert bits_equal_f32(m.hidden_states(xg), h), "training flag changed the evaluation forward"


def bits_equal_f32(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16", "fp32"])
def test_intermediate_layers_shapes(precision):
    m, _ = build(precision, 911, depth=3, img=32)
    x = rng_tensor(912, (2, 3, 32, 32)).to(DEV)
    h = m.hidden_states(x)
    for n, idx in ((1, [2]), (2, [1, 2]), (3, [0, 1, 2]), ([0, -1], [0, 2]), ((1,), [1]), ([-3, 0, 2, 2], [0, 2])):
        for reshape in (False, True):
            for prefix in (False, True):
                for norm in (False, True):
                    out = m.get_intermediate_layers(x, n=n, reshape=reshape, return_prefix_tokens=prefix, norm=norm)
                    assert isinstance(out, tuple) and len(out) == len(idx)
                    for o, l in zip(out, idx):
                        patches, cls = o if prefix else (o, None)
                        assert patches.shape == ((2, 384, 2, 2) if reshape else (2, 4, 384)) and patches.dtype == torch.float32
                        assert cls is None or cls.shape == (2, 1, 384)
                        if not norm:
                            want = h[l + 1][:, 1:]
                            want = want.reshape(2, 2, 2, 384).permute(0, 3, 1, 2) if reshape else want
                            assert torch.equal(patches, want)
                            assert cls is None or torch.equal(cls, h[l + 1][:, :1])
    for bad in (0, 4, [3], [-4], [], [True], 1.5):
        with pytest.raises((ValueError, TypeError)):
            m.get_intermediate_layers(x, n=bad)


def test_hidden_states_on_vit_base_and_with_lora():
    import vits
    from mfvit import lora
    mb = vits.vit_base(num_classes=3, depth=2, img_size=32).to(DEV)
    x = rng_tensor(921, (2, 3, 32, 32)).to(DEV)
    hb = mb.hidden_states(x)
    assert hb.shape == (3, 2, 5, 768) and torch.isfinite(hb).all()
    with torch.no_grad():
        assert scale_err(mb._final_norm(hb[-1]), mb.features3D(x)) < 1e-3
    m, _ = build("bf16x3", 922, depth=2, img=32)
    h0 = m.hidden_states(x)
    lora.add_lora(m, rank=4)
    assert bits_equal_f32(m.hidden_states(x), h0)            # (B = 0 at attachment: the merged weights are the base weights)
    with torch.no_grad():
        for p in m._lora.params():
            p.add_(0.05 * torch.randn_like(p))
        h1 = m.hidden_states(x)
        assert bits_equal_f32(h1[0], h0[0]) and not torch.equal(h1[1], h0[1])      # the patch embedding has no adapter; block 0 has
        assert scale_err(m._final_norm(h1[-1]), m.features3D(x)) < 1e-3


# ---------------------------------------------------------------------------------------------------- end to end
def models_and_batches(seed):
    ma, _ = build("bf16x3", seed, depth=2)
    mb, _ = build("bf16x3", seed + 1, depth=2)
    xs = [rng_tensor(seed + 10 + i, (8, 3, 224, 224)).to(DEV) for i in range(2)]
    ys = [rng_tensor(seed + 20 + i, (8, 3, 224, 224)).to(DEV) for i in range(2)]
    return ma, mb, xs, ys


def nan_err(got, ref):
    """Largest |got - ref| where both are numbers; NaN (an undefined CKA: a constant representation) must sit in the same places."""
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    d = np.abs(got - ref)
    return 0.0 if np.isnan(d).all() else float(np.nanmax(d))


def sel(h, tokens):
    h = h.cpu().numpy()
    return h if tokens == "all" else (h[:, :, 0] if tokens == "cls" else h[:, :, 1:])


@pytest.mark.parametrize("seed", [1301, 1401])
def test_cka_end_to_end(seed):
    """cka(m, m), cka(m_a, m_b) and stream_similarity against cka_ref fed the hidden states the models themselves returned (the forward's
    error cancels): two minibatches of 8 at 224^2, depth 2.  Measured: see E2E_MEASURED."""
    from mfvit import similarity
    fus = importlib.import_module("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
                                  "changemodelinputlocation_std002_sum")
    ma, mb, xs, ys = models_and_batches(seed)
    ha, hb_y, hb_x = [ma.hidden_states(x) for x in xs], [mb.hidden_states(y) for y in ys], [mb.hidden_states(x) for x in xs]
    worst = 0.0
    for tokens in ("all", "cls", "patch"):
        for unbiased in ((True, False) if tokens == "all" else (True,)):
            A, BY, BX = [sel(h, tokens) for h in ha], [sel(h, tokens) for h in hb_y], [sel(h, tokens) for h in hb_x]
            self_ = similarity.cka(ma, ma, xs, tokens=tokens, unbiased=unbiased)
            cross = similarity.cka(ma, mb, xs, tokens=tokens, unbiased=unbiased)
            pair = similarity.cka(ma, mb, list(zip(xs, ys)), tokens=tokens, unbiased=unbiased)
            assert self_.shape == cross.shape == pair.shape == (3, 3) and self_.dtype == np.float64
            errs = {"self": nan_err(self_, cka_ref.cka_matrix(A, A, unbiased)), "diag": nan_err(self_.diagonal(), np.where(np.isnan(self_.diagonal()), np.nan, 1.0)),
                    "cross": nan_err(cross, cka_ref.cka_matrix(A, BX, unbiased)), "pair": nan_err(pair, cka_ref.cka_matrix(A, BY, unbiased))}
            # (hidden state 0 of the cls view is the same row for every image - cls_token + pos_embed: its Gram is zero and its CKA 0 / 0, NaN on both sides)
            assert np.isnan(self_).any() == (tokens == "cls") and not np.isnan(self_[1:, 1:]).any()
            if tokens == "all" and unbiased:
                model = fus.Fus_CrossViT(ma, mb).to(DEV)
                s = model.stream_similarity(ma, mb, list(zip(xs, ys)))
                assert sorted(s) == ["cxr_cxr", "cxr_enh", "enh_enh"]
                errs["stream"] = max(nan_err(s["cxr_enh"], cka_ref.cka_matrix(A, BY, True)), nan_err(s["cxr_cxr"], cka_ref.cka_matrix(A, A, True)),
                                     nan_err(s["enh_enh"], cka_ref.cka_matrix(BY, BY, True)))
                assert np.array_equal(s["cxr_enh"], pair) and np.array_equal(s["cxr_cxr"], self_)
            log(f"cka e2e seed={seed} tokens={tokens} unbiased={unbiased}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
            worst = max(worst, *errs.values())
    log(f"cka e2e seed={seed}: largest |CKA - ref| = {worst:.3e} (gate {E2E_GATE:.3e})")
    assert worst <= E2E_GATE


def test_cka_cuts_large_batches_and_names_drop_last():
    from mfvit import similarity
    m, _ = build("bf16", 1501, depth=1, img=32)
    x = rng_tensor(1502, (260, 3, 32, 32)).to(DEV)
    got = similarity.cka(m, m, [x])                      # 256 + 4
    h = m.hidden_states(x[:256]).cpu().numpy(), m.hidden_states(x[256:]).cpu().numpy()
    err = float(np.abs(got - cka_ref.cka_matrix(list(h), list(h))).max())
    log(f"cka of 256 + 4 examples at 32^2: |CKA - ref| = {err:.3e} (gate {CUT_GATE:.3e})")
    assert err <= CUT_GATE
    with pytest.raises(ValueError, match="drop_last"):
        similarity.cka(m, m, [x[:259]])
    assert similarity.cka(m, m, [x[:258]], unbiased=False).shape == (2, 2)
