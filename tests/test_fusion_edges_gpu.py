"""The two-stream fusion (csrc/fusion.hip and the f32 GEMMs under it) at its batch, class, token and head edges, through the C ABI, against the
float64 oracle of oracle/ref_fusion.py evaluated at the same shapes (cases, inputs, error metric and gates: tests/fusion_edges_ref.py).

Every call runs with each output buffer and the workspace inside NaN guard bands that are checked after the call; the workspace has exactly
*_workspace_bytes and is pre-filled with NaN, so stale scratch can never reach a result; every element is compared; the inputs are compared
with clones after each call.  Measured errors are appended to the fusion parity report (test_fusion_gpu.REPORT).

Failures of the library before the fixes that came with this file (batch 513 / 640 at 6 or 12 heads: MFVIT_EINVAL from inside the forward; the
weight gradients above 512 rows by float atomics; token counts whose streaming passes outgrow the LDS) are listed in
profiles/parity/parity_fusion_edges.txt."""
import math
import os

import pytest
import torch

import fusion_edges_ref as fe
from test_fusion_gpu import REPORT     # where the fusion tests log their measured errors

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EINVAL = -22
G = 64                    # guard floats on each side of a buffer (256 bytes: the buffer keeps the allocation's alignment)
PAT = 0x7FC00ABC          # the guards' and pre-fills' NaN, compared as bits
MEASURED = {}             # quantity class -> (largest error of this session, case)


def log(msg):
    print(msg)
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")


def bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """A float32 device buffer between two guard bands; filled with the NaN pattern, or with `fill`."""

    def __init__(self, shape, fill=None):
        n = math.prod(shape)
        self.whole = torch.empty(n + 2 * G, dtype=torch.float32, device=DEV)
        bits(self.whole).fill_(PAT)
        self.t = self.whole[G:G + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def guards_ok(self):
        w = bits(self.whole)
        return bool((w[:G] == PAT).all()) and bool((w[-G:] == PAT).all())

    def untouched(self):
        return bool((bits(self.whole) == PAT).all())


def ptr(x):
    if x is None:
        return None
    return (x.t if isinstance(x, Guarded) else x).data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Run:
    """One mfvit_fusion_ex_forward (+ _backward) of a case under guards.  use_*: which optional pointers are passed; prefill: name -> tensor for
    dparams / dhw_* / dhb_* (zero otherwise: the gradients are then read back without a subtraction)."""

    def __init__(self, c, inp, use_hw=True, use_dfused=True, use_dx=True, use_df=True, prefill=None, backward=True, df_one_null=False):
        from mfvit import _lib
        from mfvit.fusion import fusion_cfg
        lib = _lib.lib()
        self.c, pm = c, int(c.pool == "mean")
        cfg = fusion_cfg(c.B, c.T, c.C, c.D, c.H)
        self.names = list(inp["params"])
        flat = torch.cat([v.flatten() for v in inp["params"].values()]).to(DEV)
        self.n = flat.numel()
        assert lib.mfvit_fusion_ex_param_count(cfg, c.L, pm) == self.n
        wsb = lib.mfvit_fusion_ex_workspace_bytes(cfg, c.L, pm)
        assert wsb > 0 and wsb % 4 == 0
        dev = dict(flat=flat, fc=inp["fc"].to(DEV), fe=inp["fe"].to(DEV), hw0=inp["hw"][0].to(DEV), hw1=inp["hw"][1].to(DEV),
                   hb0=inp["hb"][0].to(DEV), hb1=inp["hb"][1].to(DEV), dfu=inp["dout"][0].to(DEV), dxc=inp["dout"][1].to(DEV),
                   dxe=inp["dout"][2].to(DEV))
        clones = {k: v.clone() for k, v in dev.items()}
        hw = (dev["hw0"], dev["hb0"], dev["hw1"], dev["hb1"]) if use_hw else (None,) * 4
        self.ws = Guarded((wsb // 4,))
        self.fused, self.xc, self.xe = Guarded((c.B, c.C)), Guarded((c.B, c.C)), Guarded((c.B, c.C))
        self.rc_fwd = lib.mfvit_fusion_ex_forward(cfg, c.L, pm, ptr(flat), ptr(dev["fc"]), ptr(dev["fe"]), ptr(hw[0]), ptr(hw[1]), ptr(hw[2]),
                                                  ptr(hw[3]), ptr(self.ws), ptr(self.fused), ptr(self.xc), ptr(self.xe), stream())
        torch.cuda.synchronize()
        self.bufs = [self.ws, self.fused, self.xc, self.xe]
        self.rc_bwd = None
        if backward and self.rc_fwd == 0:
            pre = prefill or {}
            z = torch.zeros
            self.gp = Guarded((self.n,), pre.get("dparams", z(self.n)))
            self.dhw = [Guarded((c.C, c.D), pre.get(f"dhw{i}", z(c.C, c.D))) for i in range(2)]
            self.dhb = [Guarded((c.C,), pre.get(f"dhb{i}", z(c.C))) for i in range(2)]
            self.dfc = Guarded((c.B, c.T, c.D)) if use_df else None
            self.dfe = Guarded((c.B, c.T, c.D)) if use_df and not df_one_null else None
            self.rc_bwd = lib.mfvit_fusion_ex_backward(
                cfg, c.L, pm, ptr(flat), ptr(dev["fc"]), ptr(dev["fe"]), ptr(hw[0]), ptr(hw[2]), ptr(self.ws),
                ptr(dev["dfu"]) if use_dfused else None, ptr(dev["dxc"]) if use_dx else None, ptr(dev["dxe"]) if use_dx else None,
                ptr(self.gp), ptr(self.dfc), ptr(self.dfe), ptr(self.dhw[0]), ptr(self.dhb[0]), ptr(self.dhw[1]), ptr(self.dhb[1]), stream())
            torch.cuda.synchronize()
            self.bufs += [self.gp, self.dfc, self.dfe] + self.dhw + self.dhb
        for b in self.bufs:
            assert b is None or b.guards_ok(), "a guard band was written"
        for k, v in dev.items():
            assert torch.equal(bits(v), bits(clones[k])), f"input {k} was modified"
        self.use_hw, self.use_df = use_hw, use_df

    def results(self):
        """name -> CPU tensor, named as fusion_edges_ref.evaluate names them."""
        assert self.rc_fwd == 0 and self.rc_bwd == 0, (self.rc_fwd, self.rc_bwd)
        out = {"fused": self.fused.t}
        if self.use_hw:
            out.update({"x_cxr": self.xc.t, "x_enh": self.xe.t})
        o = 0
        for k in self.names:
            shape = self.shapes[k]
            out["d." + k] = self.gp.t[o:o + math.prod(shape)].view(shape)
            o += math.prod(shape)
        assert o == self.n
        for i, s in enumerate(("cxr", "enh")):
            out[f"d.hw_{s}"], out[f"d.hb_{s}"] = self.dhw[i].t, self.dhb[i].t
        if self.use_df:
            out["d.f_cxr"], out["d.f_enh"] = self.dfc.t, self.dfe.t
        return {k: v.detach().cpu().clone() for k, v in out.items()}


def run(c, inp=None, **kw):
    inp = inp or fe.make_inputs(c)
    r = Run(c, inp, **kw)
    r.shapes = {k: tuple(v.shape) for k, v in inp["params"].items()}
    return r


def record(c, errs, what=""):
    log(f"fusion edges {fe.case_id(c)}{what}: " + "  ".join(f"{q} {errs[q]:.2e}" for q in fe.QUANTITIES if q in errs))
    for q, e in errs.items():
        # (the gate tables of fusion_edges_ref: GATES_MEAN_1E3; GATES_XATTN differs from GATES in d.wq / d.wk only)
        key = ("mean_1e3" if c.stress == "mean_1e3" else "xattn" if "xattn" in what and q in ("d.wq", "d.wk") else "", q)
        if e > MEASURED.get(key, (-1.0, ""))[0]:
            MEASURED[key] = (e, fe.case_id(c) + what)


def parity(c):
    got = run(c).results()
    for k in ("d.f_cxr", "d.f_enh"):
        assert not torch.isnan(got[k]).any(), f"{k} is not fully written"
    errs = fe.errors(got, fe.oracle(c), c.H)
    record(c, errs)
    fe.check_gates(errs, fe.case_id(c), c)


@pytest.mark.parametrize("c", fe.batch_cases(), ids=fe.case_id)
def test_batch_edges_match_the_float64_oracle(c):
    parity(c)


@pytest.mark.parametrize("c", fe.class_cases(), ids=fe.case_id)
def test_class_edges_match_the_float64_oracle(c):
    parity(c)


@pytest.mark.parametrize("c", fe.token_cases(), ids=fe.case_id)
def test_token_edges_match_the_float64_oracle(c):
    parity(c)


@pytest.mark.parametrize("c", fe.lds_cases(), ids=fe.case_id)
def test_lds_heaviest_and_last_accepted_token_counts_match_the_float64_oracle(c):
    parity(c)


@pytest.mark.parametrize("dim,heads", list(fe.T_MAX))
def test_first_refused_token_count_launches_nothing(dim, heads):
    c = fe.Case(dim, heads, 1, "cls", 1, fe.T_MAX[(dim, heads)] + 1, 3)
    from mfvit import _lib
    from mfvit.fusion import fusion_cfg
    lib, cfg = _lib.lib(), fusion_cfg(c.B, c.T, c.C, c.D, c.H)
    assert lib.mfvit_fusion_ex_workspace_bytes(cfg, 1, 0) == 0 and lib.mfvit_fusion_workspace_bytes(cfg) == 0
    inp = fe.make_inputs(c)
    flat = torch.cat([v.flatten() for v in inp["params"].values()]).to(DEV)
    fc, fe_ = inp["fc"].to(DEV), inp["fe"].to(DEV)
    # every buffer has the size a launch would need: twice the last accepted token count's workspace covers one token more
    ws = Guarded((2 * lib.mfvit_fusion_ex_workspace_bytes(fusion_cfg(c.B, c.T - 1, c.C, c.D, c.H), 1, 0) // 4,))
    outs = [Guarded((c.B, c.C)) for _ in range(3)]
    grads = [Guarded((flat.numel(),)), Guarded((c.B, c.T, c.D)), Guarded((c.B, c.T, c.D))]
    d = inp["dout"][0].to(DEV)
    assert lib.mfvit_fusion_ex_forward(cfg, 1, 0, ptr(flat), ptr(fc), ptr(fe_), None, None, None, None, ptr(ws), ptr(outs[0]), ptr(outs[1]),
                                       ptr(outs[2]), stream()) == EINVAL
    assert lib.mfvit_fusion_ex_backward(cfg, 1, 0, ptr(flat), ptr(fc), ptr(fe_), None, None, ptr(ws), ptr(d), None, None, ptr(grads[0]),
                                        ptr(grads[1]), ptr(grads[2]), None, None, None, None, stream()) == EINVAL
    torch.cuda.synchronize()
    assert all(b.untouched() for b in [ws] + outs + grads)


@pytest.mark.parametrize("C", [0, 65])
def test_refused_class_counts_write_nothing(C):
    from mfvit import _lib
    from mfvit.fusion import fusion_cfg
    lib, cfg = _lib.lib(), fusion_cfg(3, 9, C)
    for L, pm in ((1, 0), (2, 1)):
        assert lib.mfvit_fusion_ex_param_count(cfg, L, pm) == 0 and lib.mfvit_fusion_ex_workspace_bytes(cfg, L, pm) == 0
    assert lib.mfvit_fusion_param_count(cfg) == 0 and lib.mfvit_fusion_workspace_bytes(cfg) == 0
    inp = fe.make_inputs(fe.Case(384, 3, 2, "mean", 3, 9, 65))
    flat = torch.cat([v.flatten() for v in inp["params"].values()]).to(DEV)
    fc, fe_, d = inp["fc"].to(DEV), inp["fe"].to(DEV), inp["dout"][0].to(DEV)
    ws = Guarded((2 * lib.mfvit_fusion_ex_workspace_bytes(fusion_cfg(3, 9, 64), 2, 1) // 4,))      # (what 64 classes need, twice)
    outs = [Guarded((3, 65)) for _ in range(3)]
    grads = [Guarded((flat.numel(),)), Guarded((3, 9, 384)), Guarded((3, 9, 384))]
    for L, pm in ((1, 0), (2, 1)):
        assert lib.mfvit_fusion_ex_forward(cfg, L, pm, ptr(flat), ptr(fc), ptr(fe_), None, None, None, None, ptr(ws), ptr(outs[0]),
                                           ptr(outs[1]), ptr(outs[2]), stream()) == EINVAL
        assert lib.mfvit_fusion_ex_backward(cfg, L, pm, ptr(flat), ptr(fc), ptr(fe_), None, None, ptr(ws), ptr(d), None, None, ptr(grads[0]),
                                            ptr(grads[1]), ptr(grads[2]), None, None, None, None, stream()) == EINVAL
    torch.cuda.synchronize()
    assert all(b.untouched() for b in [ws] + outs + grads)


# ------------------------------------------------------------------------------------------------------------ optional pointers, accumulation
OPT_CASES = [fe.Case(384, 3, 1, "cls", 3, 9, 3), fe.Case(768, 12, 1, "cls", 3, 9, 3), fe.Case(384, 6, 2, "mean", 3, 9, 3)]


@pytest.mark.parametrize("c", OPT_CASES, ids=fe.case_id)
def test_optional_pointers(c):
    inp = fe.make_inputs(c)
    # no backbone heads: x_* stay untouched, dhw_* / dhb_* receive nothing
    pre = {f"dhw{i}": fe.rng_tensor(70 + i, (c.C, c.D)) for i in range(2)}
    pre.update({f"dhb{i}": fe.rng_tensor(72 + i, (c.C,)) for i in range(2)})
    r = run(c, inp, use_hw=False, prefill=pre)
    assert r.xc.untouched() and r.xe.untouched()
    for i in range(2):
        assert torch.equal(r.dhw[i].t.cpu(), pre[f"dhw{i}"]) and torch.equal(r.dhb[i].t.cpu(), pre[f"dhb{i}"])
    got = r.results()
    for k in [k for k in got if k.startswith(("d.hw_", "d.hb_"))]:
        del got[k]
    errs = fe.errors(got, fe.evaluate(c, inp, use_hw=False), c.H)
    record(c, errs, " hw=NULL")
    fe.check_gates(errs, "hw = NULL")
    # dfused = NULL, dx_* = NULL, df_* = NULL
    for what, kw in (("dfused=NULL", dict(use_dfused=False)), ("dx=NULL", dict(use_dx=False)), ("df=NULL", dict(use_df=False))):
        got = run(c, inp, **kw).results()
        ref = fe.evaluate(c, inp, **{k: v for k, v in kw.items() if k != "use_df"})
        errs = fe.errors(got, ref, c.H)
        record(c, errs, " " + what)
        fe.check_gates(errs, what)
        if what == "dx=NULL":
            assert all(float(got[k].abs().max()) == 0.0 for k in got if k.startswith(("d.hw_", "d.hb_")))
    # one of df_cxr / df_enh NULL: refused, nothing written
    pre = {"dparams": fe.rng_tensor(74, (r.n,))}
    r = run(c, inp, df_one_null=True, prefill=pre)
    assert r.rc_fwd == 0 and r.rc_bwd == EINVAL
    assert torch.equal(r.gp.t.cpu(), pre["dparams"]) and r.dfc.untouched()


@pytest.mark.parametrize("c", OPT_CASES, ids=fe.case_id)
def test_gradients_accumulate_into_prefilled_buffers(c):
    """dparams, dhw_*, dhb_* = pre-fill + gradient.  The gradient alone is the zero-pre-fill run's; an element receives it in at most two adds
    (the fixed-order reduce adds its total to the destination once per launch), each rounded to half an ulp of its result: the bound is
    2^-23 (|pre-fill| + |gradient|) per element, worked out from the number format, not measured."""
    inp = fe.make_inputs(c)
    base = run(c, inp)
    g0 = base.results()
    pre = {"dparams": fe.rng_tensor(80, (base.n,))}
    pre.update({f"dhw{i}": fe.rng_tensor(81 + i, (c.C, c.D)) for i in range(2)})
    pre.update({f"dhb{i}": fe.rng_tensor(83 + i, (c.C,)) for i in range(2)})
    r = run(c, inp, prefill=pre)
    got = r.results()
    flat0 = torch.cat([g0["d." + k].flatten() for k in r.names])
    flat1 = torch.cat([got["d." + k].flatten() for k in r.names])
    pairs = [(flat1, pre["dparams"], flat0)]
    for i, s in enumerate(("cxr", "enh")):
        pairs += [(got[f"d.hw_{s}"], pre[f"dhw{i}"], g0[f"d.hw_{s}"]), (got[f"d.hb_{s}"], pre[f"dhb{i}"], g0[f"d.hb_{s}"])]
    for out, p, g in pairs:
        out, p, g = out.double(), p.double(), g.double()
        assert bool(((out - (p + g)).abs() <= 2.0 ** -23 * (p.abs() + g.abs())).all())
    for k in ("fused", "x_cxr", "x_enh", "d.f_cxr", "d.f_enh"):
        assert torch.equal(got[k], g0[k])


# ------------------------------------------------------------------------------------------------------------ inputs that stress the arithmetic
@pytest.mark.parametrize("c", fe.stress_cases(), ids=fe.case_id)
def test_stressed_inputs_match_the_float64_oracle(c):
    """The oracle defines the expected values; the samples beside the stressed one equal their clean run bit for bit (outputs and feature
    gradients are per sample).  A NaN in one sample's features reaches no other sample: the NaN sample itself and the batch-summed parameter
    gradients (NaN in the oracle too) are left out of that case's comparison."""
    got = run(c).results()
    others = [b for b in range(c.B) if b != fe.STRESS_SAMPLE]
    if c.stress == "nan":
        errs = fe.errors(got, fe.oracle(c), c.H, samples=others, skip_params=True)
    else:
        errs = fe.errors(got, fe.oracle(c), c.H)
    record(c, errs)
    fe.check_gates(errs, fe.case_id(c), c)
    clean = run(c._replace(stress=None)).results()
    for k in ("fused", "x_cxr", "x_enh", "d.f_cxr", "d.f_enh"):
        assert not torch.isnan(got[k][others]).any(), k
        assert torch.equal(bits(got[k][others]), bits(clean[k][others])), k


# ------------------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("B", [33, 513])
@pytest.mark.parametrize("D,H", [(384, 3), (384, 12), (768, 3), (768, 12)])
def test_two_runs_on_fresh_workspaces_give_the_same_bits(D, H, B):
    c = fe.Case(D, H, 1, "cls", B, 5, 3)
    inp = fe.make_inputs(c)
    a, b = run(c, inp).results(), run(c, inp).results()
    diff = [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]
    assert not diff, f"not reproducible: {diff}"


# ------------------------------------------------------------------------------------------------------------ stand-alone cross-attention
def xattn_case(D, H, B, T, bare):
    """A guarded run of mfvit_prenorm_xattn_* (x_own != x_oth) or mfvit_xattn_* (bare) against fusion_edges_ref.xattn_evaluate."""
    from mfvit import _lib
    from mfvit.fusion import fusion_cfg
    lib, cfg = _lib.lib(), fusion_cfg(B, T, 3, D, H)
    xi = fe.xattn_inputs(D, H, B, T, bare)
    c, p32, x_own, x_oth, dout = xi["case"], xi["params"], xi["x_own"], xi["x_oth"], xi["dout"]
    ref = fe.xattn_evaluate(xi)
    # library
    flat = torch.cat([v.flatten() for v in p32.values()]).to(DEV)
    dx_o, dx_t, dd = x_own.to(DEV), x_oth.to(DEV), dout.to(DEV)
    clones = [t.clone() for t in (flat, dx_o, dx_t, dd)]
    ws = Guarded((lib.mfvit_fusion_workspace_bytes(cfg) // 4,))
    out, gp = Guarded((B, D)), Guarded((flat.numel(),), torch.zeros(flat.numel()))
    fill = fe.rng_tensor(fe.seed_of(c) + 12, (2, B, T, D))
    g_own, g_oth = Guarded((B, T, D), fill[0]), Guarded((B, T, D), fill[1])
    if bare:
        rc = [lib.mfvit_xattn_forward(cfg, ptr(flat), ptr(dx_o), ptr(ws), ptr(out), stream()),
              lib.mfvit_xattn_backward(cfg, ptr(flat), ptr(dx_o), ptr(ws), ptr(dd), ptr(gp), ptr(g_own), stream())]
    else:
        rc = [lib.mfvit_prenorm_xattn_forward(cfg, ptr(flat), ptr(dx_o), ptr(dx_t), ptr(ws), ptr(out), stream()),
              lib.mfvit_prenorm_xattn_backward(cfg, ptr(flat), ptr(dx_o), ptr(dx_t), ptr(ws), ptr(dd), ptr(gp), ptr(g_own), ptr(g_oth), stream())]
    torch.cuda.synchronize()
    assert rc == [0, 0], rc
    assert all(b.guards_ok() for b in (ws, out, gp, g_own, g_oth))
    for t, cl in zip((flat, dx_o, dx_t, dd), clones):
        assert torch.equal(bits(t), bits(cl)), "an input was modified"
    got = {"fused": out.t.cpu()}
    o = 0
    for k, v in p32.items():
        got["d." + k] = gp.t[o:o + v.numel()].view(v.shape).cpu()
        o += v.numel()
    if bare:
        got["d.f_cxr"] = g_own.t.cpu()
    else:
        # dx_own receives row 0 only, dx_oth rows 1 .. only: what was there before stays
        assert torch.equal(g_own.t[:, 1:].cpu(), fill[0][:, 1:]) and torch.equal(g_oth.t[:, :1].cpu(), fill[1][:, :1])
        got["d.f_cxr"] = torch.cat((g_own.t[:, :1], g_oth.t[:, 1:]), 1).cpu()
    errs = fe.errors(got, ref, H)
    record(c, errs, " xattn" if bare else " prenorm_xattn")
    fe.check_gates(errs, "stand-alone cross-attention", gates=fe.GATES_XATTN)


@pytest.mark.parametrize("D,H,B,T", fe.XATTN_GRID)
def test_prenorm_xattn_with_distinct_streams(D, H, B, T):
    xattn_case(D, H, B, T, bare=False)


@pytest.mark.parametrize("D,H,B,T", fe.XATTN_GRID)
def test_bare_xattn(D, H, B, T):
    xattn_case(D, H, B, T, bare=True)


def test_zz_measured_maxima_are_logged():
    """Last in the file: the largest error of this session per quantity class beside its gate, in the parity report."""
    for tab, gates in (("", fe.GATES), ("xattn", fe.GATES_XATTN), ("mean_1e3", fe.GATES_MEAN_1E3)):
        for q in fe.QUANTITIES:
            if (tab, q) in MEASURED:
                e, where = MEASURED[(tab, q)]
                log(f"fusion edges MAX{' [' + tab + ']' if tab else ''} {q}: measured {e:.2e} ({where})  gate {gates[q]:.0e}")
