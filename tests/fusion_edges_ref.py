"""Shared by tests/test_fusion_edges_cpu.py and tests/test_fusion_edges_gpu.py: the edge cases of the two-stream fusion (batch, classes, tokens,
heads), their seeded inputs, the float64 oracle evaluated on them (oracle/ref_fusion.py, autograd on the CPU), the per-tensor error metric and the
gates.  Test infrastructure only.

Error metric: max |got - ref| / max |ref| over one tensor - with the cls row (row 0) and the patch rows (1 ..) of d f_cxr / d f_enh scaled
separately (they differ in scale: a wrong patch row would hide under the cls row), and every head's row block of d wq / d wk / d wv scaled
separately.  Every element is compared.  The errors of a case are folded into quantity classes (QUANTITIES), one gate per class.

Gates: 4 x the largest error measured on an MI355X over every case of tests/test_fusion_edges_gpu.py, rounded up to one significant digit
(profiles/parity/parity_fusion_edges.txt holds the measured maxima beside the float32 floors: the same restatement evaluated in float32 on the
CPU).  The margin covers other reduction orders across batch, tokens and head chunking.  tests/test_fusion_edges_cpu.py asserts that every
floor stays under its gate.  Two sets of cases are ill-conditioned in float32 itself and keep gates of their own, so that they do not loosen the
rest: GATES_XATTN (d wq / d wk of the stand-alone entry points at one sample) and GATES_MEAN_1E3."""
import collections
import functools
import zlib

import torch

from conftest import rng_tensor
from oracle import ref_fusion

Case = collections.namedtuple("Case", "D H L pool B T C stress", defaults=(None,))

QUANTITIES = ("out", "d.norm", "d.wq", "d.wk", "d.wv", "d.proj.weight", "d.proj.bias", "d.post", "d.head.weight", "d.head.bias", "d.hw", "d.hb",
              "df.row0", "df.rows")
# Gate per quantity class: 4 x the MI355X maximum over every case of tests/test_fusion_edges_gpu.py, rounded up to one significant digit.
# Beside each: that maximum and the float32 CPU floor (profiles/parity/parity_fusion_edges.txt has the cases they come from).
GATES = {
    "out": 3e-6,             # measured 5.62e-07  floor 1.1e-06
    "d.norm": 5e-6,          # measured 1.22e-06  floor 1.4e-06
    "d.wq": 2e-5,            # measured 4.16e-06  floor 4.2e-06
    "d.wk": 2e-5,            # measured 4.20e-06  floor 4.4e-06
    "d.wv": 5e-6,            # measured 1.22e-06  floor 1.2e-06
    "d.proj.weight": 4e-6,   # measured 9.31e-07  floor 1.6e-06
    "d.proj.bias": 5e-6,     # measured 1.03e-06  floor 1.1e-06
    "d.post": 7e-6,          # measured 1.62e-06  floor 1.6e-06
    "d.head.weight": 2e-6,   # measured 4.22e-07  floor 6.7e-07
    "d.head.bias": 2e-6,     # measured 3.45e-07  floor 5.7e-07
    "d.hw": 9e-7,            # measured 2.07e-07  floor 5.8e-07
    "d.hb": 2e-6,            # measured 4.40e-07  floor 4.0e-07
    "df.row0": 3e-6,         # measured 6.50e-07  floor 7.5e-07
    "df.rows": 4e-6,         # measured 9.62e-07  floor 1.9e-06
}
# The stand-alone entry points (mfvit_prenorm_xattn_*, mfvit_xattn_*) share GATES except for d wq / d wk: their grid has ONE sample with TWO
# tokens, where a head's score gradient is ds = a_0 a_1 (da_0 - da_1), a difference of two nearly equal numbers with no other sample to carry
# the block's scale.  The bare form at (B 1, T 2, 12 heads) measures 2.24e-05 (d wq) and 2.50e-05 (d wk) on the MI355X.  The cancellation shows
# in float32 on the CPU as well: the floor over the same grid (tests/test_fusion_edges_cpu.py asserts it under these gates) is 1.19e-05 /
# 1.18e-05 for the bare form and 9.5e-06 / 9.5e-06 behind the PreNorm, all at (B 1, T 2, 12 heads), against 1e-06 in every other class.
# 4 x 2.50e-05 is the 1e-4 no gate may exceed.
GATES_XATTN = dict(GATES, **{"d.wq": 9e-5, "d.wk": 1e-4})
# The "mean_1e3" stress (token rows of mean 1e3 and unit spread) has gates of its own, set by the same rule.  Its LayerNorm input is
# ill-conditioned: x - mean cancels three of the seven digits a float32 holds, so ANY float32 evaluation of the pre-norm is off by about
# 1e3 x 2^-24 = 6e-5 of the row's spread, and every quantity downstream of it inherits that - the float32 CPU floor of this case is 1e-5 .. 1e-4,
# 30 x the floor of every other case.  Folding it into GATES would loosen every other case's check by that factor.
# Findings: d.norm, d.wq, d.wk, d.wv, d.proj.weight and df.rows land above 1e-4 - these are the quantities that read the pre-normed rows
# z_t = LN(x_t) directly (sums over t of z_t times a gradient, or the LayerNorm backward of those rows), so they carry the 6e-5 of z_t itself;
# the straight form has the same error (the float32 floors beside them are as large or larger), so it is neither the folded algebra nor a kernel.
# The float32 floor of d.post (6.9e-05) sits within 2 % of its gate (7e-05): the CPU assertion for that class has next to no margin.
GATES_MEAN_1E3 = {
    "out": 6e-7,             # measured 1.37e-07  floor 3.1e-07
    "d.norm": 2e-4,          # measured 3.75e-05  floor 6.1e-05
    "d.wq": 4e-4,            # measured 7.92e-05  floor 9.8e-05
    "d.wk": 3e-4,            # measured 6.95e-05  floor 8.7e-05
    "d.wv": 3e-4,            # measured 5.28e-05  floor 9.2e-05
    "d.proj.weight": 4e-4,   # measured 7.95e-05  floor 8.5e-05
    "d.proj.bias": 3e-5,     # measured 6.25e-06  floor 7.5e-06
    "d.post": 7e-5,          # measured 1.71e-05  floor 6.9e-05
    "d.head.weight": 3e-5,   # measured 7.37e-06  floor 1.2e-05
    "d.head.bias": 2e-7,     # measured 3.85e-08  floor 3.8e-08
    "d.hw": 6e-7,            # measured 1.42e-07  floor 1.1e-07
    "d.hb": 2e-7,            # measured 3.70e-08  floor 3.7e-08
    "df.row0": 8e-5,         # measured 1.79e-05  floor 1.6e-05
    "df.rows": 2e-4,         # measured 4.83e-05  floor 3.8e-05
}

DEFAULT = [(384, 3), (384, 6), (384, 12), (768, 3), (768, 12)]          # (dim, heads) on the default path: one layer, pool='cls'
FULL = [(384, 6), (768, 12)]                                            # ... and on the full-row path: L = 2, pool='mean'


def case_id(c):
    return f"d{c.D}_h{c.H}_L{c.L}_{c.pool}_B{c.B}_T{c.T}_C{c.C}" + (f"_{c.stress}" if c.stress else "")


def batch_cases():
    out = []
    for B in (1, 31, 32, 33, 130, 512, 513, 640):
        for D, H in DEFAULT:
            if B != 640 or (D, H) in ((384, 3), (384, 12)):
                out.append(Case(D, H, 1, "cls", B, 5, 3))
        if B != 640:
            out += [Case(D, H, 2, "mean", B, 5, 3) for D, H in FULL]
    return out


def class_cases():
    return [Case(D, 3, L, pool, 3, 9, C) for C in (1, 2, 5, 63, 64) for D in (384, 768) for L, pool in ((1, "cls"), (2, "mean"))]


def token_cases():
    out = []
    for T in (2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129):
        out += [Case(D, H, 1, "cls", 2, T, 3) for D, H in ((384, 3), (768, 3), (384, 12), (768, 12))]
        out.append(Case(384, 6, 2, "mean", 2, T, 3))
    return out


# Largest token count whose streaming passes fit the 160 KB of LDS they may request (include/mfvit.h), from the launch code:
#   backward 32 T + 160 dim bytes; token gradient of heads > 3: 4 (max(2 heads dim + 2 heads T, 16 dim) + 2 T) bytes, = (8 heads + 8) T + 8 heads dim here
#   (768, 12): min(1280, (163840 - 73728) / 104 = 866.4)   (768, 3): (163840 - 122880) / 32 = 1280   (384, 3): (163840 - 61440) / 32 = 3200
T_MAX = {(768, 12): 866, (768, 3): 1280, (384, 3): 3200}


def lds_cases():
    return [Case(768, 12, 1, "cls", 1, 577, 3)] + [Case(D, H, 1, "cls", 1, T, 3) for (D, H), T in T_MAX.items()]


STRESSES = ("constant_row", "mean_1e3", "saturated", "tied", "denormal", "nan")


def stress_cases():
    return [Case(D, H, L, pool, 4, 17, 3, s) for s in STRESSES for D, H, L, pool in ((384, 3, 1, "cls"), (768, 12, 1, "cls"), (384, 6, 2, "mean"))]


def all_parity_cases():
    return batch_cases() + class_cases() + token_cases() + lds_cases() + stress_cases()


def seed_of(c):
    return 50000 + zlib.crc32(case_id(c._replace(stress=None)).encode()) % 40000


STRESS_SAMPLE = 2     # the sample of the batch of 4 that carries the stressed rows


def make_inputs(c):
    """float32 inputs of a case (the oracle reads the same float32 values, widened): params (name -> tensor, arena order), fc, fe, hw / hb
    of the two backbone heads, and the output gradients dfused, dxc, dxe."""
    s = seed_of(c)
    p = ref_fusion.seeded_fusion_ex_params(s, c.D, c.C, c.L)
    # Scores of unit spread at both widths (seeded_fusion_ex_params alone gives them a standard deviation of 0.0036 dim: 1.4 / 2.8), so that no
    # head's softmax saturates by chance.  A saturated head's d wq / d wk block is the residue of a cancelled sum (ds = a (da - sum a da)), 1e-4
    # of the other heads' scale and rounding noise in ANY float32 evaluation, the CPU floor included - it would set the gate of every other case.
    # Saturation is a case of its own: the "saturated" stress.
    for k, v in p.items():
        if k.endswith("fn.wq.weight"):
            v *= 0.7 * 384 / c.D
    fc, fe = rng_tensor(s + 1, (c.B, c.T, c.D)), rng_tensor(s + 2, (c.B, c.T, c.D))
    hw = [rng_tensor(s + 3 + i, (c.C, c.D), 0.05) for i in range(2)]
    hb = [rng_tensor(s + 5 + i, (c.C,), 0.1) for i in range(2)]
    dout = [rng_tensor(s + 7 + i, (c.B, c.C)) for i in range(3)]
    if c.stress:
        b = STRESS_SAMPLE
        if c.stress == "constant_row":          # variance 0: rstd = eps^-1/2
            fc[b, 3] = 0.5
            fe[b, 0] = -0.25
        elif c.stress == "mean_1e3":            # mean 1e3, unit spread
            fc[b] += 1e3
            fe[b, 5:9] += 1e3
        elif c.stress == "saturated":           # one token far along its own direction: some head's softmax puts probability 1 on it (float32)
            fc[b, 4] *= 60.0
            fe[b, 7] *= 60.0
        elif c.stress == "tied":                # two identical tokens: tied scores
            fc[b, 6] = fc[b, 2]
            fe[b, 9] = fe[b, 1]
        elif c.stress == "denormal":
            fc[b] *= 1e-39
            fe[b, 1:] *= 1e-41
        elif c.stress == "nan":
            fc[b, 2, 7] = float("nan")
            fe[b, 0, 1] = float("nan")
        else:
            raise ValueError(c.stress)
    return dict(params=p, fc=fc, fe=fe, hw=hw, hb=hb, dout=dout)


def evaluate(c, inp, dtype=torch.float64, use_hw=True, use_dfused=True, use_dx=True):
    """The restatement and its gradients in `dtype` on the CPU: name -> tensor, outputs as "fused" / "x_cxr" / "x_enh", gradients as "d." + name
    (parameters by state-dict name, "d.hw_cxr" .. "d.hb_enh", "d.f_cxr", "d.f_enh")."""
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in inp["params"].items()}
    fc, fe = (inp[k].detach().clone().to(dtype).requires_grad_(True) for k in ("fc", "fe"))
    hw = [t.detach().clone().to(dtype).requires_grad_(True) for t in inp["hw"]]
    hb = [t.detach().clone().to(dtype).requires_grad_(True) for t in inp["hb"]]
    r = [t.to(dtype) for t in inp["dout"]]
    heads = dict(hw_cxr=hw[0], hb_cxr=hb[0], hw_enh=hw[1], hb_enh=hb[1]) if use_hw else {}
    fused, xc, xe = ref_fusion.fus_ex_forward(p, fc, fe, c.H, c.L, c.pool, 1, **heads)
    loss = (fused * r[0]).sum() * (1.0 if use_dfused else 0.0)
    if use_hw and use_dx:
        loss = loss + (xc * r[1]).sum() + (xe * r[2]).sum()
    loss.backward()
    out = {"fused": fused.detach()}
    if use_hw:
        out.update({"x_cxr": xc.detach(), "x_enh": xe.detach()})
    zero = torch.zeros_like
    out.update({"d." + k: (v.grad if v.grad is not None else zero(v)) for k, v in p.items()})
    for i, s in enumerate(("cxr", "enh")):
        out[f"d.hw_{s}"] = hw[i].grad if hw[i].grad is not None else zero(hw[i])
        out[f"d.hb_{s}"] = hb[i].grad if hb[i].grad is not None else zero(hb[i])
    out["d.f_cxr"], out["d.f_enh"] = fc.grad, fe.grad
    return out


@functools.lru_cache(maxsize=None)
def oracle(c):
    """float64 oracle of a parity case with every optional pointer given (computed once, shared, never modified)."""
    return evaluate(c, make_inputs(c))


def quantity_of(name):
    if name in ("fused", "x_cxr", "x_enh"):
        return "out"
    if name in ("d.f_cxr", "d.f_enh"):
        return "df"
    if name.startswith("d.hw_"):
        return "d.hw"
    if name.startswith("d.hb_"):
        return "d.hb"
    if name.startswith("d.mlp_head_"):
        return "d.head." + name.rsplit(".", 1)[1]
    for k in ("wq", "wk", "wv"):
        if name.endswith(f"fn.{k}.weight"):
            return "d." + k
    if name.endswith("fn.proj.weight") or name.endswith("fn.proj.bias"):
        return "d.proj." + name.rsplit(".", 1)[1]
    if name.endswith("norm.weight") or name.endswith("norm.bias"):
        return "d.norm"
    return "d.post"


def scaled(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    if got.numel() == 0:
        return 0.0
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def errors(got, ref, heads, samples=None, skip_params=False):
    """Quantity class -> the largest scaled error over its tensors.  `got` may hold fewer names than `ref` (absent optional outputs).
    samples: restrict the per-sample tensors (outputs, d f_*) to these batch indices; skip_params: leave the batch-summed gradients out."""
    out = collections.defaultdict(float)

    def put(q, e):
        if e != e:
            e = float("inf")
        out[q] = max(out[q], e)
    for name, g in got.items():
        r, q = ref[name], quantity_of(name)
        if q in ("out", "df"):
            if samples is not None:
                g, r = g[samples], r[samples]
            if q == "out":
                put(q, scaled(g, r))
            else:
                put("df.row0", scaled(g[:, 0], r[:, 0]))
                put("df.rows", scaled(g[:, 1:], r[:, 1:]))
        elif skip_params:
            continue
        elif q in ("d.wq", "d.wk", "d.wv"):
            dh = r.shape[0] // heads
            for h in range(heads):
                put(q, scaled(g[h * dh:(h + 1) * dh], r[h * dh:(h + 1) * dh]))
        else:
            put(q, scaled(g, r))
    return dict(out)


def fold(total, errs):
    for q, e in errs.items():
        total[q] = max(total.get(q, 0.0), e)
    return total


def gates_for(c):
    return GATES_MEAN_1E3 if c is not None and c.stress == "mean_1e3" else GATES


def check_gates(errs, what, c=None, gates=None):
    gates = gates or gates_for(c)
    bad = {q: (e, gates[q]) for q, e in errs.items() if not e < gates[q]}
    assert not bad, f"{what}: scaled error above its gate (error, gate): {bad}"


# ------------------------------------------------------------------------------------------------------------ stand-alone cross-attention
XATTN_GRID = [(D, H, B, T) for D in (384, 768) for H in (6, 12) for B in (1, 33) for T in (2, 17)]


def xattn_inputs(D, H, B, T, bare):
    """float32 inputs of a stand-alone case: mfvit_prenorm_xattn_* with x_own != x_oth, or mfvit_xattn_* (bare: no PreNorm, one x).
    params in the entry point's arena order."""
    c = Case(D, H, 1, "cls", B, T, 3)
    inp = make_inputs(c)
    blk = ref_fusion.layer_prefix(0) + "0."
    names = ([] if bare else ["norm.weight", "norm.bias"]) + ["fn.wq.weight", "fn.wk.weight", "fn.wv.weight", "fn.proj.weight", "fn.proj.bias"]
    return dict(case=c, bare=bare, params={n: inp["params"][blk + n] for n in names}, x_own=inp["fc"], x_oth=inp["fc"] if bare else inp["fe"],
                dout=rng_tensor(seed_of(c) + 11, (B, D)))


def xattn_evaluate(xi, dtype=torch.float64):
    """oracle.ref_fusion.xattn_block and its gradients in `dtype`, named for errors(): "fused" = the output, "d." + parameter,
    "d.f_cxr" = the row gradients the entry point writes (row 0 of dx_own, rows 1 .. of dx_oth; bare: dx)."""
    H, bare = xi["case"].H, xi["bare"]
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in xi["params"].items()}
    xo, xt = (xi[k].detach().clone().to(dtype).requires_grad_(True) for k in ("x_own", "x_oth"))
    y = ref_fusion.xattn_block(p, "", xo, xo if bare else xt, H, prenorm=not bare)
    (y * xi["dout"].to(dtype)).sum().backward()
    out = {"fused": y.detach()}
    out.update({"d." + k: v.grad for k, v in p.items()})
    out["d.f_cxr"] = xo.grad if bare else torch.cat((xo.grad[:, :1], xt.grad[:, 1:]), 1)
    return out
