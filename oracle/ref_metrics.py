"""TEST INFRASTRUCTURE ONLY (see oracle/__init__.py): CPU restatement of the epoch metrics of the CA / single-stream drivers.

Follows the reference's evaluation code, MAIN_CA = main_vit_covid_..._crossvit_2vits_2additionaloutputs_trainval_sum.py:
  * `_, preds = torch.max(output, 1)`                                   MAIN_CA:870   (first maximum wins)
  * `all_gt_one_hot = label_binarize(all_gt, classes=[0,1,2])`          MAIN_CA:901
  * per class `metrics.roc_curve(onehot[:, i], all_val[:, i])` + `metrics.auc(fpr, tpr)`, mean over the 3 classes   MAIN_CA:905-909
  * `epoch_acc = sum(all_pred == all_gt) / num_imgs`, `epoch_loss = running_loss / num_imgs`                         MAIN_CA:910-911
The ROC arithmetic itself lives in scikit-learn (reference dependency, unpinned); its published algorithm - thresholds at the
distinct scores in decreasing order, cumulative TP / FP counts, trapezoid area - is restated here with integers: the area equals
(2 * #{(pos, neg): s_pos > s_neg} + #{(pos, neg): s_pos == s_neg}) / (2 * n_pos * n_neg).  tests/test_oracle_golden.py pins this
restatement against the installed sklearn.metrics.roc_curve / auc on seeded scores with ties.
"""
import numpy as np


def argmax_first(scores):
    """torch.max(output, 1)[1] / np.argmax: index of the first maximum of each row."""
    return np.argmax(scores, axis=1)


def confusion_matrix(preds, labels, num_classes):
    """conf[t][p] = number of samples with label t predicted as p.  A label outside [0, num_classes) is in no row (sklearn's confusion_matrix with
    labels=range(num_classes) drops it too); auc_pair_counts counts such a sample as a negative of every class, as label_binarize makes it."""
    conf = np.zeros((num_classes, num_classes), dtype=np.int64)
    for t, p in zip(labels.tolist(), preds.tolist()):
        if 0 <= t < num_classes:
            conf[t][p] += 1
    return conf


def auc_pair_counts(scores, labels, num_classes):
    """Per class c: (u2, n_pos, n_neg) with u2 = 2 * #{pos > neg} + #{pos == neg} over all (positive, negative) pairs."""
    out = []
    for c in range(num_classes):
        s = scores[:, c]
        pos, neg = s[labels == c], s[labels != c]
        neg_sorted = np.sort(neg)
        lt = np.searchsorted(neg_sorted, pos, side="left")      # negatives strictly below each positive
        le = np.searchsorted(neg_sorted, pos, side="right")     # negatives below or equal
        u2 = int(2 * lt.sum() + (le - lt).sum())
        out.append((u2, int(pos.size), int(neg.size)))
    return out


def auc_pair_counts_brute(scores, labels, num_classes):
    """The same triples by the definition itself: every (positive, negative) pair compared, O(n^2).  A second, independent statement - no sort, no
    search - and the definition where sorting has none: a NaN score compares neither above nor equal and adds nothing, +-inf order like numbers,
    +0.0 == -0.0, and distinct float32 denormals stay distinct."""
    out = []
    for c in range(num_classes):
        s = scores[:, c]
        pos, neg = s[labels == c], s[labels != c]
        gt = int((pos[:, None] > neg[None, :]).sum())
        eq = int((pos[:, None] == neg[None, :]).sum())
        out.append((2 * gt + eq, int(pos.size), int(neg.size)))
    return out


def roc_auc_ovr(scores, labels, num_classes):
    """Per-class one-vs-rest ROC AUC (MAIN_CA:905-907) and their mean (MAIN_CA:909).  NaN for a class without both kinds."""
    aucs = []
    for u2, npos, nneg in auc_pair_counts(scores, labels, num_classes):
        aucs.append(u2 / (2.0 * npos * nneg) if npos and nneg else float("nan"))
    return np.array(aucs), float(np.mean(aucs))


def epoch_metrics(all_val, all_gt, loss_sum, num_imgs, num_classes=3):
    """(epoch_loss, epoch_auc, epoch_acc) exactly as MAIN_CA:909-911 combines them."""
    preds = argmax_first(all_val)
    _, auc = roc_auc_ovr(all_val, all_gt, num_classes)
    return loss_sum / num_imgs, auc, float(np.sum(preds == all_gt)) / num_imgs


# ---------------------------------------------------------------------------------------------------------------------------------------
# Hard inputs for the metrics kernels, shared by tests/test_oracle_golden.py (this file against scikit-learn) and tests/test_metrics_gpu.py.
SCORE_KINDS = ("gauss", "ties", "equal", "zeros", "denormal", "inf")      # "inf" is not for scikit-learn: it rejects non-finite scores
LABEL_KINDS = ("random", "missing", "single", "outside")
OUTSIDE_LABELS = (-1, None, 2 ** 32 + 1)                                  # None stands for C itself; 2^32 + 1 is class 1 once truncated to 32 bits


def edge_scores(n, C, kind, seed):
    """float32 [n, C]: 'gauss' N(0, 1); 'ties' quantised to halves (a dozen distinct values: ties between positives and negatives everywhere, at
    every block and chunk boundary, and tied row maxima); 'equal' one value throughout; 'zeros' only +0.0 and -0.0 (equal) beside a few +-1;
    'denormal' n C distinct float32 denormals (equal only if flushed to zero); 'inf' gauss with +inf and -inf sprinkled in."""
    rng = np.random.Generator(np.random.PCG64(seed))
    s = rng.standard_normal((n, C)).astype(np.float32)
    if kind == "ties":
        s = (np.round(s * 2) / 2).astype(np.float32)
    elif kind == "equal":
        s[:] = 0.25
    elif kind == "zeros":
        s = np.where(s > 1.2, np.float32(1), np.where(s < -1.2, np.float32(-1), np.where(s > 0, np.float32(0.0), np.float32(-0.0)))).astype(np.float32)
    elif kind == "denormal":
        assert n * C < 2 ** 23
        s = rng.permutation(np.arange(1, n * C + 1, dtype=np.int32)).view(np.float32).reshape(n, C) * np.where(s > 0, np.float32(1), np.float32(-1))
    elif kind == "inf":
        u = rng.random((n, C))
        s[u < 0.1], s[u > 0.9] = np.float32("inf"), np.float32("-inf")
    return np.ascontiguousarray(s, dtype=np.float32)


def edge_labels(n, C, kind, seed):
    """int64 [n]: 'random' imbalanced classes; 'missing' the last class has no sample; 'single' class 0 holds every sample; 'outside' a third of the
    labels are -1, C or 2^32 + 1 - out of range: in no row of the confusion matrix, negatives of every class."""
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    p = np.arange(C, 0, -1, dtype=np.float64)
    t = rng.choice(C, size=n, p=p / p.sum()).astype(np.int64)
    if kind == "missing":
        t[t == C - 1] = C - 2 if C > 1 else -1
    elif kind == "single":
        t[:] = 0
    elif kind == "outside":
        out = np.array([C if v is None else v for v in OUTSIDE_LABELS], dtype=np.int64)
        pick = rng.random(n) < 1 / 3
        pick[:min(n, 3)] = n >= 3                                          # each of the three at least once where there is room
        t[pick] = out[np.arange(n) % 3][pick]
    return t
