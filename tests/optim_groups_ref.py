"""References and cases of the group-aware optimizer steps (csrc/optim.hip: adam_groups_kernel / sgd_groups_kernel; mfvit.optim with
single_launch=True, param_groups_layer_decay, ModelEma), shared by tests/test_optim_groups_cpu.py and tests/test_optim_groups_gpu.py.

The float64 reference is oracle/ref_optim.py's adam_step / sgd_step applied table row by table row, each row with the hyper entry it names.
tests/test_optim_groups_cpu.py pins it to torch.optim.AdamW / SGD built from the same groups and shows that the GPU test's gate sees a row
that took its neighbour's entry.  Hyperparameters cross the C ABI as floats: an entry holds the ROUNDED values, and those are what the
reference restates (tests/test_optim_kernels_gpu.py)."""
import numpy as np
import torch

CHUNK = 1 << 14
CAP = 64                                          # MFVIT_OPTIM_GROUPS_PER_LAUNCH: hyper entries per launch
ENTRY_COUNTS = (1, 2, CAP, CAP + 1)
ENTRY_STEPS = (1, 2, 1000)                        # an entry's step number at the first of the three steps
EINVAL = -22
LAYER_DECAY = 0.75


PIN = 1e-12                                       # float64 restatement against torch.optim, as tests/test_step_refs_cpu.py pins its references


def f32(x):
    return float(np.float32(x))


def rel(got, want):
    """max |got - want| / max |want|: the relative error of tests/test_step_refs_cpu.py's pins (an element that cancels to nearly nothing in
    beta1 m + (1 - beta1) g carries the rounding of its terms, not of itself); NaN counts as infinite."""
    got, want = got.detach().double(), want.detach().double()
    if bool(torch.isnan(got).any()):
        return float("inf")
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def adam_entries(n, decoupled):
    """n Adam entries that differ in lr (x 0.75 from one to the next, as layer decay has it), weight decay (every third one 0), the decoupled bit
    (every fourth one is the other kind) and the step number."""
    return [dict(lr=f32(1e-2 * LAYER_DECAY ** (k % 7)), beta1=f32(0.9 - 0.01 * (k % 2)), beta2=f32(0.999), eps=f32(1e-8),
                 weight_decay=0.0 if k % 3 == 1 else f32(0.1 + 0.01 * (k % 5)), decoupled=bool(decoupled) ^ (k % 4 == 3), step=ENTRY_STEPS[k % 3])
            for k in range(n)]


def sgd_entries(n, momentum):
    return [dict(lr=f32(0.1 * LAYER_DECAY ** (k % 7)), momentum=f32(momentum), weight_decay=0.0 if k % 3 == 1 else f32(0.01 + 0.001 * (k % 5)))
            for k in range(n)]


def row_entries(nrows, nentries, pattern):
    """The entry every table row names.  'interleaved': neighbouring rows name different entries; 'adjacent': runs of two rows per entry.
    Row 0 names the LAST entry either way, so with CAP + 1 entries the second launch has work."""
    if pattern == "interleaved":
        return [(nentries - 1 - r) % nentries for r in range(nrows)]
    return [(nentries - 1 - r // 2) % nentries for r in range(nrows)]


def rows_of(counts):
    """(tensor, first element, count) of every table row, tensors in order, CHUNK elements per row."""
    return [(t, a, min(CHUNK, c - a)) for t, c in enumerate(counts) for a in range(0, c, CHUNK)]


def adam_rows_ref(rows, entry_of_row, entries, P, G, M, V, step_offset=0, shift=0):
    """float64 Adam / AdamW over per-tensor 1-D tensors, row by row with the row's entry (`shift`: the entry index every row takes is off by
    that much - the mutation).  Returns new lists (P, M, V)."""
    from oracle import ref_optim
    out = [[x.double().clone() for x in X] for X in (P, M, V)]
    for (t, a, c), k in zip(rows, entry_of_row):
        e = entries[(k + shift) % len(entries)]
        s = slice(a, a + c)
        r = ref_optim.adam_step(P[t][s], G[t][s], M[t][s], V[t][s], e["step"] + step_offset, e["lr"], e["beta1"], e["beta2"], e["eps"],
                                e["weight_decay"], decoupled=e["decoupled"])
        for o, x in zip(out, r):
            o[t][s] = x
    return out


def sgd_rows_ref(rows, entry_of_row, entries, P, G, B, shift=0):
    """float64 SGD (a zero buffer is the first step: first_step=False throughout, as the kernel runs it).  Returns (P, B)."""
    from oracle import ref_optim
    out = [[x.double().clone() for x in X] for X in (P, B)]
    for (t, a, c), k in zip(rows, entry_of_row):
        e = entries[(k + shift) % len(entries)]
        s = slice(a, a + c)
        p, b = ref_optim.sgd_step(P[t][s], G[t][s], B[t][s], e["lr"], e["momentum"], e["weight_decay"], first_step=False)
        out[0][t][s] = p
        if e["momentum"] != 0:
            out[1][t][s] = b
    return out


def adam_hyper(entries, step_offset=0):
    """The ctypes array mfvit_adam_step_groups takes."""
    from mfvit import _lib
    hy = (_lib.AdamGroup * len(entries))()
    for h, e in zip(hy, entries):
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = e["lr"], e["beta1"], e["beta2"], e["eps"], e["weight_decay"]
        h.step, h.decoupled = e["step"] + step_offset, int(e["decoupled"])
    return hy


def sgd_hyper(entries):
    from mfvit import _lib
    hy = (_lib.SgdGroup * len(entries))()
    for h, e in zip(hy, entries):
        h.lr, h.momentum, h.weight_decay = e["lr"], e["momentum"], e["weight_decay"]
    return hy


def entries_of_groups(groups, steps, decoupled=True, betas=(0.9, 0.999), eps=1e-8):
    """Adam entries of optimizer param groups as the C ABI receives them (floats), `steps`: the step number of each group."""
    return [dict(lr=f32(g["lr"]), beta1=f32(betas[0]), beta2=f32(betas[1]), eps=f32(eps), weight_decay=f32(g["weight_decay"]), decoupled=decoupled,
                 step=s) for g, s in zip(groups, steps)]


# ------------------------------------------------------------------------------------------------ six groups over nine tensors
SIX_GROUPS = [[0, 1], [2], [3, 4], [5], [6], [7, 8]]          # parameter indices of ARENA_SHAPES (tests/test_optim_kernels_gpu.py); 3 is FROZEN
SIX_LR = [1e-2 * LAYER_DECAY ** (5 - i) for i in range(6)]
SIX_WD = [0.1, 0.0, 0.05, 0.1, 0.0, 0.02]
BASE_LR, EPOCHS, WARMUP = 1e-2, 10, 2
SCHEDULE_EPOCHS = (0.5, 3.0, 7.25)                            # warm-up, cosine, cosine: the lr before each of the three steps


def six_groups(params, **extra):
    return [dict(params=[params[i] for i in idx], lr=lr, lr_scale=lr / BASE_LR, weight_decay=wd, **extra) for idx, lr, wd in zip(SIX_GROUPS, SIX_LR, SIX_WD)]


# ------------------------------------------------------------------------------------------------ schedule and EMA restatements
def lr_at(epoch, lr, epochs, warmup_epochs, cos=True, schedule=()):
    """mfvit.schedules.adjust_learning_rate's value, restated (MAIN_MOCO:608-623)."""
    import math
    if cos:
        if epoch < warmup_epochs:
            return lr * epoch / warmup_epochs
        return lr * 0.5 * (1.0 + math.cos(math.pi * (epoch - warmup_epochs) / (epochs - warmup_epochs)))
    out = lr
    for milestone in schedule:
        out *= 0.1 if epoch >= milestone else 1.0
    return out


def ema_decay(t, decay, warmup):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def ema_ref(ema, w, d):
    """One float64 update and its float32 error bound 4 * 2^-24 * (|ema| d + |w| (1 - d)): the rounding of 1 - d, two products and a sum."""
    e, w = ema.double(), w.double()
    return e * d + w * (1.0 - d), 4 * 2.0 ** -24 * (e.abs() * d + w.abs() * (1.0 - d))
