"""GPU: epoch metrics kernels through the C ABI, bit-exact against oracle/ref_metrics.py."""
import numpy as np
import pytest
import torch

from oracle import ref_metrics

pytestmark = pytest.mark.gpu


def _case(n, quant, seed, C=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    scores = rng.standard_normal((n, C)).astype(np.float32)
    if quant:
        scores = (np.round(scores * quant) / quant).astype(np.float32)      # exact ties, incl. tied row maxima
    labels = rng.choice(C, size=n, p=[0.6, 0.3, 0.1] if C == 3 else None).astype(np.int64)
    return scores, labels


@pytest.mark.parametrize("n,quant", [(1, None), (5, 1), (257, None), (1000, 4), (4099, 8)])
def test_eval_counts_bit_exact(n, quant):
    from mfvit import metrics
    scores, labels = _case(n, quant, seed=100 + n)
    dev = torch.device("cuda:0")
    conf, preds, u2, npos = metrics.eval_counts(torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev))
    want_preds = ref_metrics.argmax_first(scores)
    np.testing.assert_array_equal(preds.cpu().numpy(), want_preds)                      # first maximum wins (torch.max, MAIN_CA:870)
    np.testing.assert_array_equal(conf.cpu().numpy(), ref_metrics.confusion_matrix(want_preds, labels, 3))
    pairs = ref_metrics.auc_pair_counts(scores, labels, 3)
    assert u2.cpu().tolist() == [p[0] for p in pairs]                                     # integers: bit-exact
    assert npos.cpu().tolist() == [p[1] for p in pairs]


def test_epoch_meter_matches_reference_epoch_arithmetic():
    """EpochMeter over several ragged batches == the oracle's restatement of MAIN_CA:884-911 on the concatenated epoch."""
    from mfvit import metrics
    dev = torch.device("cuda:0")
    scores, labels = _case(777, 16, seed=5)
    meter = metrics.EpochMeter(3)
    loss_sum, i = 0.0, 0
    for bs in (128, 128, 128, 128, 128, 128, 9):
        s, t = scores[i:i + bs], labels[i:i + bs]
        loss = torch.nn.functional.cross_entropy(torch.from_numpy(s), torch.from_numpy(t))
        loss_sum += float(loss) * len(t)                                                  # running_loss += loss.item() * n
        meter.update(torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev).float(), loss.to(dev))   # labels arrive as float, MAIN_CA:856
        i += bs
    got = meter.compute()
    want = ref_metrics.epoch_metrics(scores, labels, loss_sum, 777)
    assert abs(got[0] - want[0]) < 1e-6 * abs(want[0])
    assert abs(got[1] - want[1]) < 1e-12 and abs(got[2] - want[2]) < 1e-12
    per, _ = ref_metrics.roc_auc_ovr(scores, labels, 3)
    np.testing.assert_allclose(meter.auc_per_class.numpy(), per, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the C ABI at its edges
# mfvit_eval_counts through ctypes: what include/mfvit.h promises and the tests above never ask for - a row stride, either half NULL, accumulation
# across calls, the first maximum "as torch.max" (NaN included), labels outside [0, C) - at the sizes where the kernels' loops turn over: the
# 256-sample block and the 1,024-score LDS chunk, each minus one, exact and plus one.  Every integer is compared bit for bit.
DEV = "cuda:0"
N_EDGES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
EXTRA = 3                                  # NaN columns beside the C scores: ld = C + 3, and an over-read of a row is poisoned
SENTINEL = -0x0123456789ABCDEF             # what the guard words around every integer output hold
GUARD = 8


def _guarded_int(numel, fill=0):
    """(buffer, view): `numel` int64 words (zeroed: the outputs accumulate) between GUARD sentinel words on either side"""
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL, device=DEV, dtype=torch.int64)
    buf[GUARD:GUARD + numel] = fill
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _counts(scores, labels, want_conf=True, want_preds=True, want_auc=True, into=None):
    """One mfvit_eval_counts call on `scores` laid out as the column slice wide[:, :C] of a NaN-filled [n, C + EXTRA] tensor.  Returns the four output
    views (conf [C, C], preds, u2, npos; all int64) - the guarded buffers are kept in `into` and reused when it is handed in again."""
    from mfvit._lib import check, lib, ptr, stream
    n, C = scores.shape
    wide = torch.full((n, C + EXTRA), float("nan"), device=DEV)
    wide[:, :C] = torch.from_numpy(scores).to(DEV)
    view, lab = wide[:, :C], torch.from_numpy(labels).to(DEV)
    assert view.stride(0) == C + EXTRA and view.data_ptr() == wide.data_ptr()
    wide0, lab0 = wide.clone(), lab.clone()
    st = into if into else dict(conf=_guarded_int(C * C), preds=_guarded_int(n, SENTINEL), u2=_guarded_int(C), npos=_guarded_int(C))
    if into is not None:
        into.update(st)
    check(lib().mfvit_eval_counts(ptr(view), view.stride(0), ptr(lab), n, C, ptr(st["conf"][1]) if want_conf else None,
                                  ptr(st["preds"][1]) if want_preds else None, ptr(st["u2"][1]) if want_auc else None,
                                  ptr(st["npos"][1]) if want_auc else None, stream()), "mfvit_eval_counts")
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int32), wide0.view(torch.int32)) and torch.equal(lab, lab0)          # inputs are read-only
    assert all(_guards_intact(b) for b, _ in st.values())
    return st["conf"][1].view(C, C).cpu().numpy(), st["preds"][1].cpu().numpy(), st["u2"][1].cpu().tolist(), st["npos"][1].cpu().tolist()


def _check_counts(scores, labels, got, what):
    C = scores.shape[1]
    conf, preds, u2, npos = got
    want_preds = ref_metrics.argmax_first(scores)
    np.testing.assert_array_equal(preds, want_preds, err_msg=str(what))
    np.testing.assert_array_equal(conf, ref_metrics.confusion_matrix(want_preds, labels, C), err_msg=str(what))
    finite = bool(np.isfinite(scores).all())
    pairs = ref_metrics.auc_pair_counts(scores, labels, C) if finite else ref_metrics.auc_pair_counts_brute(scores, labels, C)
    assert u2 == [p[0] for p in pairs] and npos == [p[1] for p in pairs], what
    return pairs


@pytest.mark.parametrize("C", [1, 2, 3, 5])
def test_eval_counts_strided_scores_hard_values_and_labels_at_block_and_chunk_edges(C):
    seen = set()
    for i, n in enumerate(N_EDGES):
        for k, kind in enumerate(ref_metrics.SCORE_KINDS):
            lkind = ref_metrics.LABEL_KINDS[(i + k) % len(ref_metrics.LABEL_KINDS)]
            seen.add((kind, lkind))
            scores, labels = ref_metrics.edge_scores(n, C, kind, 31 * n + C), ref_metrics.edge_labels(n, C, lkind, 31 * n + C)
            pairs = _check_counts(scores, labels, _counts(scores, labels), (n, kind, lkind))
            if kind == "equal":                                          # every pair a tie: u2 == npos * nneg exactly, the AUC 0.5
                assert all(u2 == npos * nneg for u2, npos, nneg in pairs)
            if kind == "denormal" and n > 1 and lkind == "random" and C > 1:      # distinct denormals stay distinct: no pair is a tie
                assert all(u2 % 2 == 0 for u2, _, _ in pairs)
    assert {k for k, _ in seen} == set(ref_metrics.SCORE_KINDS) and {l for _, l in seen} == set(ref_metrics.LABEL_KINDS)


def test_eval_counts_ties_straddle_the_1024_score_chunk():
    """Positives and negatives with the same score on both sides of the chunk boundary: samples 1020..1027 all hold one value, the labels alternate."""
    n, C = 1100, 2
    scores = ref_metrics.edge_scores(n, C, "gauss", 3)
    scores[1020:1028] = 0.125
    labels = (np.arange(n) % 2).astype(np.int64)
    _check_counts(scores, labels, _counts(scores, labels), "chunk boundary")


def test_eval_counts_with_a_thousand_classes():
    """grid.y = C: the encoder's default head has 1,000 classes"""
    n, C = 300, 1000
    for kind, lkind in (("gauss", "random"), ("ties", "outside")):
        scores, labels = ref_metrics.edge_scores(n, C, kind, 77), ref_metrics.edge_labels(n, C, lkind, 77)
        _check_counts(scores, labels, _counts(scores, labels), (kind, lkind))


def test_eval_counts_labels_outside_the_classes_are_compared_in_64_bits():
    """-1, C and 2^32 + 1 are nobody's class: in no row of the confusion matrix, negatives of every class.  (2^32 + 1 truncated to 32 bits is class 1.)"""
    C = 3
    scores = ref_metrics.edge_scores(6, C, "gauss", 5)
    labels = np.array([0, 1, 2, -1, C, 2 ** 32 + 1], dtype=np.int64)
    conf, preds, u2, npos = got = _counts(scores, labels)
    _check_counts(scores, labels, got, "outside labels")
    assert conf.sum() == 3 and npos == [1, 1, 1]
    assert conf[1].sum() == 1                                             # row 1 holds sample 1 alone


def test_eval_counts_first_maximum_with_nan_is_torch_max():
    """include/mfvit.h, "First maximum": the first NaN of a row wins, otherwise the first of the largest values - torch.max(x, 1)[1], np.argmax."""
    rows = np.array([[1, np.nan, 3], [np.nan, 2, 1], [3, 1, np.nan], [2, 5, 5], [np.nan, np.nan, 7], [-np.inf, -np.inf, -np.inf], [0.0, -0.0, 0.0]],
                    dtype=np.float32)
    rng = np.random.Generator(np.random.PCG64(9))
    more = rng.standard_normal((600, 3)).astype(np.float32)
    more[rng.random((600, 3)) < 0.2] = np.nan
    scores = np.concatenate([rows, more])
    labels = rng.integers(0, 3, size=len(scores)).astype(np.int64)
    conf, preds, _, _ = _counts(scores, labels, want_auc=False)
    assert preds[:7].tolist() == [1, 0, 2, 1, 0, 0, 0]
    want = torch.from_numpy(scores).max(1)[1].numpy()
    np.testing.assert_array_equal(want, ref_metrics.argmax_first(scores))
    np.testing.assert_array_equal(preds, want)
    np.testing.assert_array_equal(conf, ref_metrics.confusion_matrix(want, labels, 3))


def test_eval_counts_either_half_null_and_accumulation_across_calls():
    from mfvit._lib import lib, ptr, stream
    C = 5
    sa, la = ref_metrics.edge_scores(300, C, "ties", 1), ref_metrics.edge_labels(300, C, "outside", 1)
    sb, lb = ref_metrics.edge_scores(1025, C, "gauss", 2), ref_metrics.edge_labels(1025, C, "random", 2)
    pa, pb = ref_metrics.argmax_first(sa), ref_metrics.argmax_first(sb)
    ca, cb = ref_metrics.confusion_matrix(pa, la, C), ref_metrics.confusion_matrix(pb, lb, C)
    ua, ub = ref_metrics.auc_pair_counts(sa, la, C), ref_metrics.auc_pair_counts(sb, lb, C)
    # confusion NULL: the pair counts alone; conf and preds (written by the confusion half) stay as they were
    conf, preds, u2, npos = _counts(sa, la, want_conf=False)
    assert not conf.any() and (preds == SENTINEL).all() and u2 == [p[0] for p in ua] and npos == [p[1] for p in ua]
    # u2 / npos NULL: the confusion matrix and preds alone
    conf, preds, u2, npos = _counts(sa, la, want_auc=False)
    np.testing.assert_array_equal(conf, ca)
    np.testing.assert_array_equal(preds, pa)
    assert not any(u2) and not any(npos)
    # preds NULL
    conf, preds, u2, npos = _counts(sa, la, want_preds=False)
    np.testing.assert_array_equal(conf, ca)
    assert (preds == SENTINEL).all() and u2 == [p[0] for p in ua]
    # two calls into the same arrays add up (the pair counts are per call: their sum is the sum of the two calls' counts)
    keep = {}
    _counts(sa, la, into=keep)
    keep["preds"] = _guarded_int(len(lb), SENTINEL)
    conf, preds, u2, npos = _counts(sb, lb, into=keep)
    np.testing.assert_array_equal(conf, ca + cb)
    np.testing.assert_array_equal(preds, pb)
    assert u2 == [a[0] + b[0] for a, b in zip(ua, ub)] and npos == [a[1] + b[1] for a, b in zip(ua, ub)]
    # nothing to compute is an invalid call, not a silent success
    s, l = torch.zeros(4, C, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    assert lib().mfvit_eval_counts(ptr(s), C, ptr(l), 4, C, None, None, None, None, stream()) != 0
    assert lib().mfvit_eval_counts(ptr(s), C, ptr(l), 4, C, None, None, ptr(l), None, stream()) != 0


def test_epoch_meter_five_classes_bf16_logits_float_labels():
    """One epoch at C = 5 in ragged batches, the logits in bf16 and the labels as floats (MAIN_CA:856), a class that never occurs: EpochMeter
    against the oracle's epoch arithmetic on the float32 values of the same bf16 logits."""
    from mfvit import metrics
    n, C = 1500, 5
    logits = torch.from_numpy(ref_metrics.edge_scores(n, C, "ties", 21)).to(torch.bfloat16)
    labels = ref_metrics.edge_labels(n, C, "random", 21)
    scores = logits.float().numpy()
    meter = metrics.EpochMeter(C)
    loss_sum, i = 0.0, 0
    for bs in (256, 1, 255, 257, 512, 219):
        s, t = logits[i:i + bs], torch.from_numpy(labels[i:i + bs])
        loss = torch.nn.functional.cross_entropy(s.float(), t)
        loss_sum += float(loss) * bs
        meter.update(s.to(DEV), t.to(DEV).float(), loss.to(DEV))
        i += bs
    assert i == n
    got = meter.compute()
    want = ref_metrics.epoch_metrics(scores, labels, loss_sum, n, C)
    assert abs(got[0] - want[0]) < 1e-6 * abs(want[0])
    assert abs(got[1] - want[1]) < 1e-12 and abs(got[2] - want[2]) < 1e-12
    per, _ = ref_metrics.roc_auc_ovr(scores, labels, C)
    np.testing.assert_allclose(meter.auc_per_class.numpy(), per, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(meter.confusion.numpy(), ref_metrics.confusion_matrix(ref_metrics.argmax_first(scores), labels, C))
    # a class without a sample: its AUC is NaN and so is the mean, without an exception (as the oracle and scikit-learn's auc of NaN rates)
    meter.reset()
    labels = ref_metrics.edge_labels(n, C, "missing", 21)
    meter.update(logits.to(DEV), torch.from_numpy(labels).to(DEV).float(), torch.zeros((), device=DEV))
    _, auc, acc = meter.compute()
    per, _ = ref_metrics.roc_auc_ovr(scores, labels, C)
    assert np.isnan(auc) and np.isnan(per[C - 1]) and np.isnan(float(meter.auc_per_class[C - 1]))
    np.testing.assert_allclose(meter.auc_per_class.numpy()[:C - 1], per[:C - 1], rtol=0, atol=1e-12)
    assert abs(acc - float(np.sum(ref_metrics.argmax_first(scores) == labels)) / n) < 1e-12
