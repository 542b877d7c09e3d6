"""Single-kernel parity of the MoCo row kernels (csrc/moco.hip) against float64 on the same float32 inputs, through the C ABI, at the places
where their address arithmetic can go wrong:
  mfvit_cross_entropy_rows   every 16-byte phase of the row pointers (base offset x row stride), gradient rows of the same and of another phase
                             (vector / scalar stores), targets in column 0, every head and tail position, every lane of the first and last float4
                             and column C - 1, the fixed-order and the atomic loss, forward-only calls, n beyond the loss kernel's 256 sequences
  mfvit_l2norm_fwd / _bwd, mfvit_rowdot   partial 4-row blocks, C from 1 to 4096, a zero row and a row far below eps, rowdot written in place into
                             column 0 of (n, 4097) and (n, 65537) logits
  mfvit_ema_update           the float4 / scalar split at every size edge, every alignment of dst and src
Every buffer a kernel can reach is a view inside a larger tensor filled with NaN: reading a neighbour poisons the result, writing one is seen
bit for bit.  The case matrix of the cross entropy and the float64 references live in oracle/ref_moco.py; tests/test_step_refs_cpu.py pins
the references to torch and shows on the CPU that CE_GATE separates the right sweep from planted index bugs.  Measured errors are appended to
parity_moco_ops.txt, beside the parity_ops.txt of tests/test_ops_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                  # guard floats before and behind every view (a multiple of 4: the view's phase is its offset)
NAN = float("nan")

# Gate of mfvit_cross_entropy_rows on loss, lse and dlogits: max abs error over the tensor's max abs, against float64.
#   floor     the float32 restatement of the sweep with exact exp / log (oracle/ref_moco.py::ce_rows_sweep_f32) over the whole case matrix,
#             on the CPU: at most 1.1e-6, in dlogits at C = 1024 (tests/test_step_refs_cpu.py prints it per C)
#   expected  __expf / __logf scale their argument by log2(e) in float32: about |x| 2^-24 relative per element at |x| <= 40, 2.4e-6
#   measured  on an MI355X over the 960 cases: fixed-order loss 5.4e-7, lse 5.6e-8, dlogits 1.1e-6 (C = 1024), atomic loss 2.8e-6 (C = 2: 300 row
#             losses added by float atomics in arrival order)
#   gate      no more than 4 x the largest measured error (1.1e-5), one significant digit; 2e-5 is the ceiling above which an error is a finding
CE_GATE = 1e-5
ROW_GATE = 2e-6           # l2norm / rowdot: float32 accumulation of at most 4096 terms per lane-strided sum (the gate of test_layernorm_fwd_bwd)


def log(msg):
    from test_ops_gpu import REPORT as OPS_REPORT              # the report directory of the single-op parity tests
    report = os.path.join(os.path.dirname(OPS_REPORT), "parity_moco_ops.txt")
    os.makedirs(os.path.dirname(report), exist_ok=True)
    with open(report, "a") as f:
        f.write(msg + "\n")


def rel_err(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    if bool(torch.isnan(got).any()):
        return float("inf")
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def guarded(numel, off=0, fill=NAN):
    """(buffer, view): `numel` floats at float offset `off` (0..3: the view's 16-byte phase) inside a NaN-filled buffer."""
    buf = torch.full((PAD + off + numel + PAD,), fill, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + off:PAD + off + numel]


def rows_view(buf, n, C, ld, off):
    return torch.as_strided(buf, (n, C), (ld, 1), PAD + off)


def same_bits(a, b, writable=None):
    a, b = a.view(torch.int32), b.view(torch.int32)
    if writable is None:
        return torch.equal(a, b)
    return torch.equal(a[~writable], b[~writable])


# ------------------------------------------------------------------------------------------------ mfvit_cross_entropy_rows
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4097, 65537])
def test_cross_entropy_rows_at_every_phase_stride_and_target_position(C):
    from conftest import rng_tensor
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_moco
    assert C in ref_moco.CE_C
    pool = rng_tensor(9000 + C, (max(ref_moco.CE_N) if C <= 4097 else ref_moco.CE_N_WIDE, C), scale=5.0)
    worst = dict(loss=0.0, lse=0.0, dlogits=0.0, loss_atomic=0.0, dlogits_atomic=0.0)
    hits, exist, dvec_seen, paths = {}, {}, {}, set()
    for case in ref_moco.ce_cases(C):
        n, off, ld, mode = case["n"], case["off"], case["ld"], case["mode"]
        z, t = ref_moco.ce_case_inputs(case, pool, hits.setdefault(off, set()))
        assert int(t.min()) >= 0 and int(t.max()) < C
        head, tail0 = ref_moco.ce_row_split(C, n, off, ld)
        for h, t0 in set(zip(head.tolist(), tail0.tolist())):
            exist.setdefault(off, set()).update(ref_moco.ce_target_classes(C, h, t0))
        span = (n - 1) * ld + C
        zbuf, _ = guarded(span, off)
        zwin = rows_view(zbuf, n, C, ld, off)
        zwin.copy_(z.to(DEV))
        assert zwin.data_ptr() % 16 == 4 * off                         # the phase arithmetic of the case matrix is the pointers' own
        tgt = t.to(DEV)
        r_loss, r_lse, r_d = ref_moco.ce_rows(zwin, tgt)
        z0 = zbuf.clone()
        want_d = mode != "null"
        if want_d:
            dspan = (n - 1) * case["ldd"] + C
            dvec = ref_moco.ce_row_dvec(case)
            dvec_seen.setdefault(off, set()).update(dvec.tolist())
            dmask = torch.zeros(PAD + case["doff"] + dspan + PAD, dtype=torch.bool, device=DEV)
            rows_view(dmask, n, C, case["ldd"], case["doff"]).fill_(True)

        def run(with_lse):
            lbuf, lwin = guarded(1, 1)
            sbuf, swin = guarded(n, 3)
            dbuf = dwin = None
            if want_d:
                dbuf, _ = guarded(dspan, case["doff"])
                dwin = rows_view(dbuf, n, C, case["ldd"], case["doff"])
                assert ((dwin.data_ptr() // 4 + torch.arange(n) * case["ldd"] + head) % 4 == 0).tolist() == dvec.tolist()
            check(lib().mfvit_cross_entropy_rows(ptr(zwin), ld, ptr(tgt), ptr(lwin), ptr(swin) if with_lse else None, ptr(dwin), case["ldd"], n, C,
                                                 stream()), "mfvit_cross_entropy_rows")
            torch.cuda.synchronize()
            assert same_bits(zbuf, z0), case                                    # the logits, and the gaps between their rows, are read-only
            keep = torch.zeros_like(lbuf, dtype=torch.bool)
            keep[PAD + 1] = True
            assert same_bits(lbuf, torch.full_like(lbuf, NAN), keep), case      # only loss_mean itself (zeroed by the entry point, then written)
            keep = torch.zeros_like(sbuf, dtype=torch.bool)
            if with_lse:
                keep[PAD + 3:PAD + 3 + n] = True
            assert same_bits(sbuf, torch.full_like(sbuf, NAN), keep), case
            if want_d:
                assert same_bits(dbuf, torch.full_like(dbuf, NAN), dmask), case    # nothing outside the [row, :C] windows
            return lwin.clone(), swin.clone(), None if dwin is None else dwin.clone()

        a = run(True)
        b = run(True)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and (not want_d or same_bits(a[2], b[2])), case     # fixed order: the same bits
        c = run(False)
        paths |= {"fixed", "atomic"}
        e = dict(loss=rel_err(a[0], r_loss.reshape(1)), lse=rel_err(a[1], r_lse), loss_atomic=rel_err(c[0], r_loss.reshape(1)))
        if want_d:
            e["dlogits"], e["dlogits_atomic"] = rel_err(a[2], r_d), rel_err(c[2], r_d)
        for k, v in e.items():
            worst[k] = max(worst[k], v)
        assert all(v < CE_GATE for v in e.values()), (case, e)
    log(f"cross_entropy_rows[C={C}, {len(ref_moco.ce_cases(C))} cases] " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  gate {CE_GATE:.0e}")
    # coverage, from the same phase arithmetic: a later change to the matrix cannot silently drop a class, a store path or a loss path
    for off in range(4):
        assert hits[off] == exist[off], (C, off, exist[off] - hits[off])
        assert {"col0", "last"} <= hits[off]
        if C >= 8:
            assert {f"{s}{i}" for s in ("head", "tail") for i in range(3)} | {f"{g}.{l}" for g in ("first", "final") for l in "xyzw"} <= hits[off]
        assert dvec_seen[off] == {True, False}, (C, off)
    assert paths == {"fixed", "atomic"}


# ------------------------------------------------------------------------------------------------ mfvit_l2norm_fwd / _bwd, mfvit_rowdot
def row_err(got, ref, scale=None):
    """max over the rows of (max abs error of the row / scale of the row): a row of 1 / eps magnitude cannot hide the others.  The scale of a row is
    its own max abs, or the one handed in where the result is a difference of larger terms."""
    got, ref = got.detach().double(), ref.detach().double()
    if bool(torch.isnan(got).any()):
        return float("inf")
    scale = ref.abs().amax(dim=1) if scale is None else scale.double()
    return float(((got - ref).abs().amax(dim=1) / scale.clamp_min(1e-30)).max())


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 100, 256, 4096])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 130])
def test_l2norm_and_rowdot_at_partial_row_blocks_and_every_width(n, C):
    from conftest import rng_tensor
    from mfvit._lib import check, lib, ptr, stream
    from oracle import ref_moco
    EPS = float(np.float32(1e-12))                                    # the float the kernel receives
    x = rng_tensor(3000 + 7 * n + C, (n, C))
    if n >= 3:
        x[1] = 0.0                                                    # y = 0, inv = 1 / eps, dx = dy / eps, as F.normalize gives
        x[2] *= 1e-20 / float(x[2].double().norm())                   # norm about 1e-20: its square is a float32 denormal
    dy = rng_tensor(3001 + 7 * n + C, (n, C))
    off = (n + C) % 4
    xbuf, xw = guarded(n * C, off)
    xw = xw.view(n, C)
    xw.copy_(x.to(DEV))
    ybuf, yw = guarded(n * C, (off + 1) % 4)
    ibuf, iw = guarded(n, 1)
    x0 = xbuf.clone()
    check(lib().mfvit_l2norm_fwd(ptr(xw), ptr(yw), ptr(iw), n, C, 1e-12, stream()), "mfvit_l2norm_fwd")
    torch.cuda.synchronize()
    yw = yw.view(n, C)
    r_y, r_inv = ref_moco.l2norm_fwd(xw, EPS)
    e = dict(y=row_err(yw, r_y), inv=float(((iw.double() - r_inv).abs() / r_inv).max()))
    assert same_bits(xbuf, x0)
    for buf, o, k in ((ybuf, (off + 1) % 4, n * C), (ibuf, 1, n)):
        m = torch.zeros_like(buf, dtype=torch.bool)
        m[PAD + o:PAD + o + k] = True
        assert same_bits(buf, torch.full_like(buf, NAN), m)
    if n >= 3:
        assert not bool(yw[1].any())                                  # (inv[1] = 1 / eps is part of e['inv'])
    # backward on the kernel's own y and inv
    gbuf, gw = guarded(n * C, (off + 2) % 4)
    gw = gw.view(n, C)
    gw.copy_(dy.to(DEV))
    dbuf, dw = guarded(n * C, (off + 3) % 4)
    y0, i0, g0 = ybuf.clone(), ibuf.clone(), gbuf.clone()
    check(lib().mfvit_l2norm_bwd(ptr(gw), ptr(yw), ptr(iw), ptr(dw), n, C, stream()), "mfvit_l2norm_bwd")
    torch.cuda.synchronize()
    # dx = (dy - y (y . dy)) / norm is a difference: at C = 1 it is zero up to the rounding of y (y = +-1), at small C it may be far smaller than
    # its terms.  What float32 can promise is a few roundings of the terms, so the scale of a row is max |dy| / norm, not max |dx|.
    e["dx"] = row_err(dw.view(n, C), ref_moco.l2norm_bwd(gw, yw, iw), gw.abs().amax(dim=1) * iw)
    assert same_bits(ybuf, y0) and same_bits(ibuf, i0) and same_bits(gbuf, g0)
    m = torch.zeros_like(dbuf, dtype=torch.bool)
    m[PAD + (off + 3) % 4:PAD + (off + 3) % 4 + n * C] = True
    assert same_bits(dbuf, torch.full_like(dbuf, NAN), m)
    if n >= 3:
        assert row_err(dw.view(n, C)[1:2], gw[1:2].double() / EPS) < ROW_GATE
    # rowdot, written in place into column 0 of the logits: keys correlated with the queries, as matched pairs are (no cancellation to zero)
    bbuf, bw = guarded(n * C, (off + 2) % 4)
    bw = bw.view(n, C)
    bw.copy_((0.5 * x + 0.1 * dy).to(DEV))
    b0 = bbuf.clone()
    for ldo in (1, 4097, 65537):
        for scale in (1.0, 1 / 0.2):
            obuf, _ = guarded((n - 1) * ldo + 1, 3)
            m = torch.zeros_like(obuf, dtype=torch.bool)
            m[PAD + 3:PAD + 3 + (n - 1) * ldo + 1:ldo] = True
            ow = torch.as_strided(obuf, (n,), (ldo,), PAD + 3)
            check(lib().mfvit_rowdot(ptr(xw), ptr(bw), ptr(ow), ldo, scale, n, C, stream()), "mfvit_rowdot")
            torch.cuda.synchronize()
            assert same_bits(obuf, torch.full_like(obuf, NAN), m), (ldo, scale)          # only column 0 of each row
            assert same_bits(xbuf, x0) and same_bits(bbuf, b0)
            k = f"rowdot[ldo={ldo},scale={scale:g}]"
            e[k] = rel_err(ow, ref_moco.rowdot(xw, bw, float(np.float32(scale))))
    log(f"l2norm / rowdot[n={n}, C={C}] " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  gate {ROW_GATE:.0e}")
    assert all(v < ROW_GATE for v in e.values()), e


# ------------------------------------------------------------------------------------------------ mfvit_ema_update
EMA_ALIGN = {"both aligned": (0, 0), "only dst aligned": (0, 1), "only src aligned": (2, 0), "both off alike": (3, 3), "both off differently": (1, 2)}


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, 4 * 256 * 3 + 2, 1 << 20 | 3])
def test_ema_update_at_every_size_edge_and_alignment(n):
    from conftest import rng_tensor
    from mfvit._lib import check, lib, ptr, stream
    d_host, s_host = rng_tensor(5000 + n % 1000, (n,)), rng_tensor(5001 + n % 1000, (n,), scale=3.0)
    worst, vector = 0.0, set()
    for name, (doff, soff) in EMA_ALIGN.items():
        for m in (0.0, 0.5, 0.99, 1.0):
            dbuf, dw = guarded(n, doff)
            sbuf, sw = guarded(n, soff)
            dw.copy_(d_host.to(DEV))
            sw.copy_(s_host.to(DEV))
            vector.add(dw.data_ptr() % 16 == 0 and sw.data_ptr() % 16 == 0 and n >= 4)
            d0, s0 = dbuf.clone(), sbuf.clone()
            check(lib().mfvit_ema_update(ptr(dw), ptr(sw), m, n, stream()), "mfvit_ema_update")
            torch.cuda.synchronize()
            keep = torch.zeros_like(dbuf, dtype=torch.bool)
            keep[PAD + doff:PAD + doff + n] = True
            assert same_bits(dbuf, d0, keep) and same_bits(sbuf, s0), (name, m)
            m32 = float(np.float32(m))
            dd, sd = d0[PAD + doff:PAD + doff + n].double(), sw.double()
            ref = dd * m32 + sd * (1.0 - m32)
            # 2 ulp of max(|d|, |s|): two or three roundings, with or without FMA contraction
            ulp = torch.ldexp(torch.ones_like(dd), torch.frexp(torch.maximum(dd.abs(), sd.abs()))[1] - 24)
            worst = max(worst, float(((dw.double() - ref).abs() / ulp).max()))
            assert bool(((dw.double() - ref).abs() <= 2 * ulp).all()), (name, m)
            if m == 1.0:
                assert same_bits(dbuf, d0), name                     # m = 1 leaves dst as it is
            if m == 0.0:
                assert same_bits(dw, sw), name                       # m = 0 copies src
    assert vector == ({True, False} if n >= 4 else {False})        # both the float4 + scalar-tail launch and the all-scalar launch ran
    log(f"ema_update[n={n}, 5 alignments x m in (0, 0.5, 0.99, 1)] max error {worst:.2f} ulp of max(|d|, |s|)  gate 2 ulp")
