"""Epoch metrics of the finetune / CA drivers on the device.

The reference copies predictions, logits and labels of every batch to the host (MAIN_CA:886-899) and calls scikit-learn at the end
of the epoch (label_binarize + roc_curve + auc per class, MAIN_CA:901-909).  `EpochMeter` keeps them in HBM; `compute()` runs two
small HIP kernels (argmax + confusion matrix, one-vs-rest AUC pair counts as exact integers) and does ONE device-to-host copy.
"""
import torch

from . import _lib
from ._lib import check, lib, ptr, require_cuda, stream


def eval_counts(scores, labels, num_classes=None):
    """scores f32 [n, C], labels int64 [n] on the GPU -> (confusion [C, C] int64, preds [n] int64, u2 [C] int64, npos [C] int64)."""
    require_cuda(scores, labels)
    if scores.dtype != torch.float32 or labels.dtype != torch.int64 or scores.dim() != 2:
        raise _lib.MfvitError("eval_counts wants float32 [n, C] scores and int64 labels")
    n, C = scores.shape
    if num_classes is not None and num_classes != C:
        raise _lib.MfvitError("scores have a different class count")
    if scores.stride(1) != 1:
        scores = scores.contiguous()
    conf = torch.zeros(C, C, device=scores.device, dtype=torch.int64)
    u2 = torch.zeros(C, device=scores.device, dtype=torch.int64)
    npos = torch.zeros(C, device=scores.device, dtype=torch.int64)
    preds = torch.empty(n, device=scores.device, dtype=torch.int64)
    check(lib().mfvit_eval_counts(ptr(scores), scores.stride(0), ptr(labels), n, C, ptr(conf), ptr(preds), ptr(u2), ptr(npos), stream()),
          "mfvit_eval_counts")
    return conf, preds, u2, npos


class EpochMeter:
    """Accumulates `output`, `target` and the summed loss of an epoch on the device; mirrors MAIN_CA:884-911.

        meter = EpochMeter(num_classes=3)
        for ...:  meter.update(output, target, loss)        # loss = the batch MEAN, as criterion() returns it (MAIN_CA:873,884)
        epoch_loss, epoch_auc, epoch_acc = meter.compute()  # no host sync before this call
    """

    def __init__(self, num_classes=3):
        self.num_classes = num_classes
        self.reset()

    def reset(self):
        self._scores, self._labels = [], []
        self._loss_sum = None
        self.confusion = None
        self.auc_per_class = None

    def update(self, output, target, loss):
        out = output.detach().float()
        self._scores.append(out)
        self._labels.append(target.detach().long().view(-1))
        w = loss.detach().float() * out.shape[0]                      # running_loss += loss.item() * images.size(0), MAIN_CA:884
        self._loss_sum = w if self._loss_sum is None else self._loss_sum + w

    def compute(self):
        scores = torch.cat(self._scores, 0).contiguous()
        labels = torch.cat(self._labels, 0).contiguous()
        n = scores.shape[0]
        conf, _, u2, npos = eval_counts(scores, labels, self.num_classes)
        host = torch.cat([conf.view(-1), u2, npos, self._loss_sum.view(1).double().view(torch.int64)]).cpu()   # one copy
        C = self.num_classes
        conf = host[:C * C].view(C, C)
        u2, npos = host[C * C:C * C + C].double(), host[C * C + C:C * C + 2 * C].double()
        loss_sum = host[-1:].view(torch.float64).item()
        nneg = n - npos
        auc = u2 / (2.0 * npos * nneg)                                # nan for a class without positives or negatives, as sklearn
        self.confusion = conf
        self.auc_per_class = auc
        return loss_sum / n, float(auc.mean()), float(conf.diag().sum()) / n

    def _epoch(self):
        return torch.cat(self._scores, 0).contiguous(), torch.cat(self._labels, 0).contiguous()

    def bootstrap_ci(self, n_boot=2000, level=0.95, seed=0, stratified=False):
        """Bootstrap percentile intervals of the epoch's metrics (mfvit.evalstats.bootstrap_ci with one score set, named "0")."""
        from . import evalstats
        scores, labels = self._epoch()
        return evalstats.bootstrap_ci(scores, labels, n_boot, level, seed, stratified)

    def delong(self, level=0.95):
        """DeLong variance and normal interval of the epoch's per-class AUC (mfvit.evalstats.delong with one score set)."""
        from . import evalstats
        scores, labels = self._epoch()
        return evalstats.delong(scores, labels, level)

    def roc_curve(self, drop_intermediate=True):
        """Per class (fpr, tpr, thresholds) of the epoch's outputs taken as scores, as compute() takes them: what MAIN_CA:904-907 gets from
        metrics.roc_curve (mfvit.evalstats.roc_curve)."""
        from . import evalstats
        scores, labels = self._epoch()
        return evalstats.roc_curve(scores, labels, drop_intermediate)

    def operating_points(self, at, n_boot=2000, level=0.95, seed=0, stratified=False):
        """Sensitivity / specificity / PPV / NPV at the operating points `at` with bootstrap intervals, the outputs taken as scores
        (mfvit.evalstats.operating_points with one score set, named "0")."""
        from . import evalstats
        scores, labels = self._epoch()
        return evalstats.operating_points(scores, labels, at, n_boot, level, seed, stratified)

    def calibration(self, temperature=1.0, n_bins=15):
        """ECE, MCE, Brier score, NLL and the reliability diagram of softmax(outputs / temperature): here the stored outputs are logits
        (mfvit.evalstats.calibration)."""
        from . import evalstats
        scores, labels = self._epoch()
        return evalstats.calibration(scores, labels, temperature, n_bins)
