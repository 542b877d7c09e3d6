"""Representation similarity: minibatch linear CKA between the hidden states of two encoders (include/mfvit.h, mfvit_gram_centered /
mfvit_hsic_accumulate; csrc/cka.hip).

Linear CKA is Kornblith et al. 2019; the minibatch estimator - HSIC summed over minibatches before the ratio is taken, with the unbiased
HSIC of Song et al. 2012 - is Nguyen, Raghu & Kornblith 2021; Raghu et al. 2021 applied it to ViTs layer by layer:

    CKA = sum_b HSIC(K_b, L_b) / sqrt(sum_b HSIC(K_b, K_b) * sum_b HSIC(L_b, L_b)),   K = X X',  L = Y Y'  over the flattened features.

The Gram matrices are taken on the GPU from f32 features whose columns are centred in LDS (both estimators are exactly invariant to that
shift; a raw f32 Gram of residual-stream features loses the signal to cancellation), the HSIC sums run in double, and the accumulators stay
on the device: one copy to the host, in result().  No CPU / eager fallback.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream

MAX_N = 256        # MFVIT_GRAM_MAX_N: rows of a minibatch
MAX_REPS = 64      # representations of one stack
TOKENS = ("all", "cls", "patch")


def _rows_view(t):
    """(tensor to read, rep_stride, ld, k) of an (R, n, ...) f32 stack: the tensor itself when a reshape to (R, n, k) is a view of it with unit
    column stride, and its strides and address are multiples of 16 bytes (a view into an encoder workspace is) - a contiguous copy otherwise."""
    R, n = t.shape[0], t.shape[1]
    k = t[0, 0].numel()
    try:
        v = t.view(R, n, k)
    except RuntimeError:
        v = None
    if v is None or v.stride(2) != 1 or v.stride(1) < k or v.stride(1) % 4 or v.stride(0) % 4 or v.stride(0) < 0 or v.data_ptr() % 16:
        v = torch.zeros(R, n, (k + 3) // 4 * 4, device=t.device, dtype=torch.float32)[:, :, :k]     # (rows of a copy start at multiples of 16 bytes)
        v.copy_(t.reshape(R, n, k))
    return v, v.stride(0), v.stride(1), k


def gram_centered(t):
    """(R, n, ...) f32 stack on the GPU -> (R, n, n) float64 centred Gram matrices (mfvit_gram_centered)."""
    _lib.require_cuda(t)
    if t.dtype != torch.float32 or t.dim() < 3:
        raise ValueError(f"expected an (R, n, ...) float32 stack, got {tuple(t.shape)} {t.dtype}")
    R, n = t.shape[0], t.shape[1]
    if not 1 <= R <= MAX_REPS or not 2 <= n <= MAX_N:
        raise ValueError(f"a stack holds 1 .. {MAX_REPS} representations of 2 .. {MAX_N} rows, got R = {R}, n = {n}")
    src, rs, ld, k = _rows_view(t)
    if k < 1:
        raise ValueError("empty features")
    nbytes = lib().mfvit_gram_work_bytes(R, n, k)
    work = torch.empty(nbytes, device=t.device, dtype=torch.uint8)
    g = torch.empty(R, n, n, device=t.device, dtype=torch.float64)
    check(lib().mfvit_gram_centered(ptr(src), rs, ld, R, n, k, ptr(g), ptr(work), nbytes, stream()), "mfvit_gram_centered")
    return g


class CKAMeter:
    """Accumulates the three HSIC sums of minibatch CKA between ra and rb representations on the device.

    update(hidden_a, hidden_b): (ra, n, ...) and (rb, n, ...) f32 stacks over the same n examples (4 <= n <= 256 with unbiased, 2 <= n
    otherwise); features past the second axis are flattened.  Views into a workspace are read in place through their base pointer, row and
    representation strides.  Nothing synchronises with the host.  result(): one copy to the host; the (ra, rb) float64 CKA matrix."""

    def __init__(self, ra, rb, unbiased=True):
        if not (1 <= ra <= MAX_REPS and 1 <= rb <= MAX_REPS):
            raise ValueError(f"1 .. {MAX_REPS} representations per side, got {ra} x {rb}")
        self.ra, self.rb, self.unbiased = int(ra), int(rb), bool(unbiased)
        self._acc = None
        self.batches = 0

    def update(self, hidden_a, hidden_b):
        if hidden_a.shape[0] != self.ra or hidden_b.shape[0] != self.rb:
            raise ValueError(f"expected stacks of {self.ra} and {self.rb} representations, got {hidden_a.shape[0]} and {hidden_b.shape[0]}")
        n = hidden_a.shape[1]
        if hidden_b.shape[1] != n:
            raise ValueError(f"both stacks must hold the same examples, got {n} and {hidden_b.shape[1]} rows")
        lo = 4 if self.unbiased else 2
        if not lo <= n <= MAX_N:
            raise ValueError(f"a minibatch of {n} examples: the {'unbiased ' if self.unbiased else ''}estimator needs {lo} .. {MAX_N} "
                             "(drop a short last minibatch: drop_last)")
        ga = gram_centered(hidden_a)
        gb = ga if hidden_b is hidden_a else gram_centered(hidden_b)
        if self._acc is None:
            self._acc = torch.zeros(self.ra * self.rb + self.ra + self.rb, device=ga.device, dtype=torch.float64)
        ab = self._acc.data_ptr()
        check(lib().mfvit_hsic_accumulate(ptr(ga), self.ra, ptr(gb), self.rb, n, int(self.unbiased), ab, ab + 8 * self.ra * self.rb,
                                          ab + 8 * (self.ra * self.rb + self.ra), stream()), "mfvit_hsic_accumulate")
        self.batches += 1

    def sums(self):
        """(sum HSIC(K, L) (ra, rb), sum HSIC(K, K) (ra,), sum HSIC(L, L) (rb,)) as float64 arrays: one copy to the host."""
        if self._acc is None:
            raise RuntimeError("CKAMeter.result() before any update()")
        a = self._acc.cpu().numpy()
        nab = self.ra * self.rb
        return a[:nab].reshape(self.ra, self.rb), a[nab:nab + self.ra], a[nab + self.ra:]

    def result(self):
        ab, aa, bb = self.sums()
        with np.errstate(invalid="ignore", divide="ignore"):
            return ab / np.sqrt(aa[:, None] * bb[None, :])


def linear_cka(x, y, unbiased=True):
    """Linear CKA of two (n, d, ...) f32 GPU tensors over the same n examples (everything past the first axis flattened): a float."""
    m = CKAMeter(1, 1, unbiased)
    m.update(x[None], y[None])
    return float(m.result()[0, 0])


def _select(h, tokens):
    """The token view of a (L + 1, n, T, D) hidden-state stack: the same buffer, another base / width."""
    if tokens == "all":
        return h
    if tokens == "cls":
        return h[:, :, 0]
    return h[:, :, 1:]


def _minibatches(batch, unbiased):
    B = batch[0].shape[0]
    if any(x.shape[0] != B for x in batch):
        raise ValueError("the inputs of one batch must hold the same number of examples")
    for s in range(0, B, MAX_N):
        n = min(MAX_N, B - s)
        if n < (4 if unbiased else 2):
            raise ValueError(f"a minibatch of {n} examples is too short for the {'unbiased ' if unbiased else ''}HSIC estimator: "
                             "drop the short last batch (drop_last=True)")
        yield [x[s:s + n] for x in batch]


def layerwise(models, batches, pairs, tokens="all", unbiased=True):
    """Minibatch CKA between the hidden states of `models` (VisionTransformerMoCo) for every (i, j) of `pairs`: a list of
    (L_i + 1, L_j + 1) float64 arrays.  `batches` yields a tensor, fed to every model, or one input per model.  One evaluation forward per
    distinct (model, input) and minibatch; its hidden states are read in place from the workspace."""
    if tokens not in TOKENS:
        raise ValueError(f"tokens must be one of {TOKENS}, got {tokens!r} (mean pooling is not built)")
    meters = [CKAMeter(models[i].depth + 1, models[j].depth + 1, unbiased) for i, j in pairs]
    for batch in batches:
        batch = [batch] * len(models) if torch.is_tensor(batch) else list(batch)
        if len(batch) != len(models):
            raise ValueError(f"a batch must be a tensor or {len(models)} inputs, got {len(batch)}")
        for xs in _minibatches(batch, unbiased):
            held, views = [], []
            try:
                for mi, (m, x) in enumerate(zip(models, xs)):
                    same = next((j for j in range(mi) if models[j] is m and batch[j] is batch[mi]), None)
                    if same is not None:
                        views.append(views[same])
                        continue
                    cfg, ws, _ = m._rel_forward(x)
                    held.append((m, ws))
                    views.append(_select(m._hidden_view(cfg, ws), tokens))
                for meter, (i, j) in zip(meters, pairs):
                    meter.update(views[i], views[j])
            finally:
                for m, ws in held:      # (stream-ordered: whoever takes the workspace next queues behind the Gram launches)
                    m._release_ws(ws)
    if not meters[0].batches:
        raise ValueError("no batch")
    return [m.result() for m in meters]


def cka(model_a, model_b, batches, tokens="all", unbiased=True):
    """(La + 1, Lb + 1) minibatch linear CKA between hidden state i of model_a and hidden state j of model_b (hidden_states' numbering).
    batches yields a tensor (fed to both models) or an (input_a, input_b) pair; batches above 256 examples are cut into minibatches of at
    most 256.  tokens: 'all' (T * D features), 'cls' (D) or 'patch' ((T - 1) * D).  model_a is model_b on the same input runs one forward."""
    return layerwise([model_a, model_b], batches, [(0, 1)], tokens, unbiased)[0]
