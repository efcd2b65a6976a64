"""The float64 preconditioner (simplex_gp_amd/csrc/plx_pcg_f64.hip) on the GPU: the four calls at every tile edge, the class
solvers.LatticePreconditioner64, and the preconditioned double solve through LatticeGP.khat_solve and
marginal_log_likelihood.

Bars are derived, never measured.  U2 = 2^-52 (the unit roundoff 2^-53 once for each side of a comparison); T is the sum of
the absolute values of the terms an entry adds up.  n - 1 additions in ANY order give at most (n - 1) u T to first order and
the products one more u each, so a bar holds for every summation tree (MFMA chain, partial sums, final tree):
  * gram entry      (n + 4) U2 Tg, Tg = sum_i |L_ij R_ic|
  * project entry   (n + kp + 8) U2 sum_q |Cinv_jq| Tg_qc (the gram sum, then kp more terms)
  * apply entry     (k + 6) U2 |s1| (|s0 r| + sum_j |L_ij T_jc|), from the device's own T
  * rz              (n + 4) U2 sum_r |R Z|, from the device's own Z
  * direction entry 4 U2 (|z| + |beta p|); beta 4 U2 relative
References are evaluated in np.longdouble (64-bit mantissa on x86) from the values the kernel received.  `pytest -s` prints
the worst ratio to its bar per kernel (report())."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
import tests.test_f64_gpu as f64t
from simplex_gp_amd import _native as nv
from simplex_gp_amd import lattice_kernel as lk
from simplex_gp_amd import solvers
from tests.gpubuf import SENTINEL, Buf, check_buffers
from tests.lattice64 import cloud
from tests.solver64 import active64, entry_ratio, rel_ratio

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -52
TINY64 = 1e-300
PLX_ERR_INVALID = 1
F64, F32 = torch.float64, torch.float32
LD = np.longdouble

NS = (1, 63, 64, 65, 255, 257, 1023, 3077)     # fewer rows than a tile, ld = n and ld > n, more tiles than waves in a workgroup
RANKS = ((1, 16), (16, 16), (17, 32), (100, 112))
TS = (1, 2, 3, 4, 11, 12, 16)

WORST = {}
REACHED = set()


def note(kernel, ratio, bar):
    REACHED.add(kernel)
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio / bar)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ld_(a):
    return np.asarray(a, LD)


def f64_(a):
    return np.asarray(a, np.float64)


def work_doubles(n, kp, t):
    return int(nv.lib().plx_pcg_work_doubles(n, kp, t))


def factor(rng, n, k, kp):
    """(host [kp][ld] fp32 with zero rows k.. and a zero tail, ld)."""
    ld = (n + 63) // 64 * 64
    lt = np.zeros((kp, ld), np.float32)
    lt[:k, :n] = rng.standard_normal((k, n)).astype(np.float32)
    return lt, ld


def direction_kernel(n, vd, off):
    return "step_direction_vec_kernel" if (n * vd) % 2 == 0 and off % 2 == 0 else "step_direction_kernel"


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("k,kp", RANKS)
@pytest.mark.parametrize("n", NS)
def test_pcg64_kernels(n, k, kp):
    """plx_pcg_gram_f64, plx_pcg_project_f64, plx_pcg_apply_f64 and plx_pcg_step_direction_f64 at one factor shape, every
    column count, R and Z 16-byte aligned and offset by one double: the bars, two calls bit-equal, guards intact.  With the
    offset buffers rows k..kp-1 of T hold a sentinel: apply reads only k."""
    lib = nv.lib()
    rng = np.random.default_rng(100000 * n + kp)
    lt, ld = factor(rng, n, k, kp)
    LT = Buf(lt, dtype=F32)
    assert LT.raw.data_ptr() % 16 == 0
    Lr = ld_(lt[:, :n])                                  # [kp][n]
    La = np.abs(Lr)
    cinv = rng.standard_normal((kp, kp)) / math.sqrt(kp)
    cinv = 0.5 * (cinv + cinv.T)
    CINV = Buf(cinv, dtype=F64)
    scale = np.array([1.25, -0.375])
    SC = Buf(scale, dtype=F64)
    for t in TS:
        for off in (0, 1):
            label = f"n={n} k={k} kp={kp} t={t} off={off}"
            r = rng.standard_normal((n, t))
            R = Buf(r, offset=off, dtype=F64)
            work = Buf(count=work_doubles(n, kp, t), offset=off, dtype=F64)
            Tg = f64_(La @ np.abs(ld_(r)))               # [kp][t]
            g_want = f64_(Lr @ ld_(r))
            # ---- gram
            outs = []
            for _ in range(2):
                G = Buf(count=kp * 16, offset=off, dtype=F64)
                nv.check(lib.plx_pcg_gram_f64(LT.ptr, ld, kp, R.ptr, n, t, G.ptr, work.ptr, stream()), "plx_pcg_gram_f64")
                check_buffers(inputs=(LT, R), outputs=(G, work))
                outs.append(G.cpu(kp, 16))
            assert torch.equal(bits(outs[0]), bits(outs[1])), (label, "gram not deterministic")
            g = outs[0].numpy()
            assert (g[:, t:] == SENTINEL).all(), (label, "gram wrote a column >= t")
            e = entry_ratio(g[:, :t], g_want, Tg)
            note("pcg64_gram_kernel", e, (n + 4) * U2)
            REACHED.add("pcg64_project_kernel")
            assert e <= (n + 4) * U2, (label, "gram", e)
            assert (g[k:, :t] == 0).all(), (label, "zero factor rows give zero sums")
            # ---- project
            outs = []
            for _ in range(2):
                Tm = Buf(count=kp * 16, offset=off, dtype=F64)
                nv.check(lib.plx_pcg_project_f64(LT.ptr, ld, kp, R.ptr, n, t, CINV.ptr, Tm.ptr, work.ptr, stream()),
                         "plx_pcg_project_f64")
                check_buffers(inputs=(LT, R, CINV), outputs=(Tm, work))
                outs.append(Tm.cpu(kp, 16))
            assert torch.equal(bits(outs[0]), bits(outs[1])), (label, "project not deterministic")
            tm = outs[0].numpy().copy()
            assert (tm[:, t:] == SENTINEL).all(), (label, "project wrote a column >= t")
            t_want = f64_(ld_(cinv) @ (Lr @ ld_(r)))
            e = entry_ratio(tm[:, :t], t_want, np.abs(cinv) @ Tg)
            note("pcg64_project_kernel", e, (n + kp + 8) * U2)
            assert e <= (n + kp + 8) * U2, (label, "project", e)
            # ---- apply (from the device's own T; off = 1: a sentinel in the rows apply must not read)
            if off == 1:
                tm[k:, :] = SENTINEL
            TM = Buf(tm, offset=off, dtype=F64)
            outs = []
            for _ in range(2):
                Z, RZ = Buf(count=n * t, offset=off, dtype=F64), Buf(count=t, offset=off, dtype=F64)
                nv.check(lib.plx_pcg_apply_f64(LT.ptr, ld, kp, k, R.ptr, n, t, TM.ptr, SC.ptr, Z.ptr, RZ.ptr, work.ptr, stream()),
                         "plx_pcg_apply_f64")
                check_buffers(inputs=(LT, R, TM, SC), outputs=(Z, RZ, work))
                outs.append((Z.cpu(n, t), RZ.cpu()))
            assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1])), \
                (label, "apply not deterministic")
            z, rz = outs[0][0].numpy(), outs[0][1].numpy()
            tk = ld_(tm[:k, :t])
            z_want = f64_((scale[0] * ld_(r) - Lr[:k].T @ tk) * scale[1])
            Tz = f64_((np.abs(scale[0] * ld_(r)) + La[:k].T @ np.abs(tk)) * abs(scale[1]))
            e = entry_ratio(z, z_want, Tz)
            kernel = f"pcg64_apply_kernel<{t}>"
            note(kernel, e, (k + 6) * U2)
            assert e <= (k + 6) * U2, (label, "apply", e)
            prod = ld_(r) * ld_(z)
            e = entry_ratio(rz, f64_(prod.sum(0)), f64_(np.abs(prod).sum(0)))
            note("coldot_final_kernel", e, (n + 4) * U2)
            assert e <= (n + 4) * U2, (label, "rz", e)
            # rz = NULL: the same Z
            Z2 = Buf(count=n * t, offset=off, dtype=F64)
            nv.check(lib.plx_pcg_apply_f64(LT.ptr, ld, kp, k, R.ptr, n, t, TM.ptr, SC.ptr, Z2.ptr, None, work.ptr, stream()),
                     "plx_pcg_apply_f64")
            assert torch.equal(bits(Z2.cpu(n, t)), bits(outs[0][0])), (label, "Z without rz")
            # ---- direction (tol far from every column's sqrt(rr) / b_norm; one column inactive)
            p0 = rng.standard_normal((n, t))
            rzn, rz0 = rng.uniform(0.5, 2.0, t) * n, rng.uniform(0.5, 2.0, t) * n
            rr = rng.uniform(0.5, 2.0, t) * n
            b_norm = np.sqrt(rr) * rng.uniform(10.0, 20.0, t)
            act = np.ones(t)
            inactive = t // 2 if t > 1 else None
            if inactive is not None:
                act[inactive] = 0.0
            tol = 1e-3
            outs = []
            for _ in range(2):
                P, Zs = Buf(p0, offset=off, dtype=F64), Buf(z, offset=off, dtype=F64)
                RZN, RZ0, RR, ACT, BN = (Buf(a, dtype=F64) for a in (rzn, rz0, rr, act, b_norm))
                beta, act_out = Buf(count=t, offset=off, dtype=F64), Buf(count=t, offset=off, dtype=F64)
                nv.check(lib.plx_pcg_step_direction_f64(P.ptr, Zs.ptr, RZN.ptr, RZ0.ptr, RR.ptr, ACT.ptr, BN.ptr, tol, n, t, beta.ptr,
                                                        act_out.ptr, stream()), "plx_pcg_step_direction_f64")
                check_buffers(inputs=(Zs, RZN, RZ0, RR, ACT, BN), outputs=(P, beta, act_out))
                outs.append((P.cpu(n, t), beta.cpu(), act_out.cpu()))
            for u, v in zip(*outs):
                assert torch.equal(bits(u), bits(v)), (label, "direction not deterministic")
            gp, gb, gact = (x.numpy() for x in outs[0])
            beta_want = np.where(act > 0, f64_(ld_(rzn) / np.maximum(ld_(rz0), TINY64)), 0.0)
            eb = rel_ratio(gb, beta_want)
            wp = f64_(ld_(z) + ld_(gb) * ld_(p0))
            ep = entry_ratio(gp, wp, np.abs(z) + np.abs(gb * p0))
            note(direction_kernel(n, t, off), max(eb, ep), 4 * U2)
            assert eb <= 4 * U2 and ep <= 4 * U2, (label, "direction", eb, ep)
            flag, decided = active64(act, rr, b_norm, tol)
            assert decided.all() and np.array_equal(gact, flag.astype(np.float64)), (label, "active_out")
            if inactive is not None:
                assert gb[inactive] == 0.0 and gact[inactive] == 0.0
                assert np.array_equal(gp[:, inactive].view(np.int64), z[:, inactive].view(np.int64)), (label, "P = Z of a frozen column")


def test_apply_large_reaches_the_unrolled_final_sum():
    """n = 786,689 at kp = 16, k = 1, t = 2: <R, Z> has 3074 partial rows (one per 256 rows), more than 3 * 1024, so
    coldot_final_kernel's four-way unrolled loop runs -- plx_coldot_f64 always hands it 1024 rows.  The <R, Z> bar of
    test_pcg64_kernels, (n + 4) U2 on the entry ratio against longdouble from the device's own Z."""
    lib = nv.lib()
    n, k, kp, t = 786_689, 1, 16, 2
    assert (n + 255) // 256 == 3074
    rng = np.random.default_rng(n)
    lt, ld = factor(rng, n, k, kp)
    assert ld == 786_752
    LT = Buf(lt, dtype=F32)
    r, tm = rng.standard_normal((n, t)), rng.standard_normal((kp, 16))
    scale = np.array([1.25, -0.375])
    R, TM, SC = Buf(r, dtype=F64), Buf(tm, dtype=F64), Buf(scale, dtype=F64)
    work = Buf(count=work_doubles(n, kp, t), dtype=F64)
    Z, RZ = Buf(count=n * t, dtype=F64), Buf(count=t, dtype=F64)
    nv.check(lib.plx_pcg_apply_f64(LT.ptr, ld, kp, k, R.ptr, n, t, TM.ptr, SC.ptr, Z.ptr, RZ.ptr, work.ptr, stream()),
             "plx_pcg_apply_f64")
    check_buffers(inputs=(LT, R, TM, SC), outputs=(Z, RZ, work))
    z, rz = Z.np(n, t), RZ.np()
    lcol, tk = ld_(lt[:k, :n]).T, ld_(tm[:k, :t])
    z_want = f64_((scale[0] * ld_(r) - lcol @ tk) * scale[1])
    Tz = f64_((np.abs(scale[0] * ld_(r)) + np.abs(lcol) @ np.abs(tk)) * abs(scale[1]))
    e = entry_ratio(z, z_want, Tz)
    note(f"pcg64_apply_kernel<{t}>", e, (k + 6) * U2)
    assert e <= (k + 6) * U2, ("apply", e)
    prod = ld_(r) * ld_(z)
    e = entry_ratio(rz, f64_(prod.sum(0)), f64_(np.abs(prod).sum(0)))
    note("coldot_final_kernel", e, (n + 4) * U2)
    print(f"<R, Z> over 3074 partial rows: error / ((n + 4) U2) = {e / ((n + 4) * U2):.4f}")
    assert e <= (n + 4) * U2, ("rz", e)


@pytest.mark.parametrize("vd", (3, 12))
@pytest.mark.parametrize("n", (1, 257))
def test_cg_direction_is_the_pcg_direction(n, vd):
    """plx_cg_step_direction_f64(P, R, rs_new, rs, ...) is plx_pcg_step_direction_f64(P, R, rs_new, rs, rr = rs_new, ...):
    P, beta and active_out agree bit for bit, buffers aligned and offset by one double (the scalar and the pair form each
    way), one column inactive and the columns on either side of tol."""
    lib = nv.lib()
    rng = np.random.default_rng(10 * n + vd)
    p0, r0 = rng.standard_normal((n, vd)), rng.standard_normal((n, vd))
    rs_new, rs = rng.uniform(0.5, 2.0, vd) * n, rng.uniform(0.5, 2.0, vd) * n
    tol = 1e-3
    b_norm = np.sqrt(rs_new) / tol * np.where(np.arange(vd) % 2 == 0, 0.5, 2.0)
    act = np.ones(vd)
    act[vd // 2] = 0.0
    for off in (0, 1):
        RSN, RS, ACT, BN = (Buf(a, dtype=F64) for a in (rs_new, rs, act, b_norm))
        outs = []
        for pcg in (False, True):
            P, R = Buf(p0, offset=off, dtype=F64), Buf(r0, offset=off, dtype=F64)
            beta, act_out = Buf(count=vd, offset=off, dtype=F64), Buf(count=vd, offset=off, dtype=F64)
            if pcg:
                nv.check(lib.plx_pcg_step_direction_f64(P.ptr, R.ptr, RSN.ptr, RS.ptr, RSN.ptr, ACT.ptr, BN.ptr, tol, n, vd,
                                                        beta.ptr, act_out.ptr, stream()), "plx_pcg_step_direction_f64")
            else:
                nv.check(lib.plx_cg_step_direction_f64(P.ptr, R.ptr, RSN.ptr, RS.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr,
                                                       act_out.ptr, stream()), "plx_cg_step_direction_f64")
            check_buffers(inputs=(R, RSN, RS, ACT, BN), outputs=(P, beta, act_out))
            outs.append((P.cpu(), beta.cpu(), act_out.cpu()))
        for name, u, v in zip(("P", "beta", "active_out"), *outs):
            assert torch.equal(bits(u), bits(v)), (n, vd, off, name)
        REACHED.add(direction_kernel(n, vd, off))
        gp, gb, gact = (x.numpy() for x in outs[0])
        assert not np.array_equal(gp, p0.reshape(-1)) and set(gact.tolist()) == {0.0, 1.0} and gb[vd // 2] == 0.0


@pytest.mark.parametrize("vd", (3, 12))
def test_direction_threshold(vd):
    """sqrt(rr) / b_norm on either side of tol by 2e-3 decides the flag (active64's decided-margin of 1e-3), whatever rz says;
    and the 1e-300 guard: rz = 0 gives a finite beta."""
    lib = nv.lib()
    n, tol = 257, 1e-6
    rng = np.random.default_rng(vd)
    b_norm = rng.uniform(1.0, 2.0, vd)
    side = np.where(np.arange(vd) % 2 == 0, 1.0 + 2e-3, 1.0 - 2e-3)
    rr = (tol * b_norm * side) ** 2
    rzn, rz = rng.uniform(0.5, 2.0, vd), rng.uniform(0.5, 2.0, vd)
    rz[1] = 0.0
    rzn[1] = 1e-295                                     # beta = 1e-295 / max(0, 1e-300) = 1e5
    act = np.ones(vd)
    P, Z = Buf(rng.standard_normal((n, vd)), dtype=F64), Buf(rng.standard_normal((n, vd)), dtype=F64)
    RZN, RZ, RR, ACT, BN = (Buf(a, dtype=F64) for a in (rzn, rz, rr, act, b_norm))
    beta, act_out = Buf(count=vd, dtype=F64), Buf(count=vd, dtype=F64)
    nv.check(lib.plx_pcg_step_direction_f64(P.ptr, Z.ptr, RZN.ptr, RZ.ptr, RR.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr,
                                            act_out.ptr, stream()), "plx_pcg_step_direction_f64")
    flag, decided = active64(act, rr, b_norm, tol, margin=1e-3)
    assert decided.all(), "the margin of 2e-3 in sqrt(rr) is outside active64's 1e-3"
    assert np.array_equal(act_out.np(), flag.astype(np.float64)) and set(flag.tolist()) == {0.0, 1.0}
    want = f64_(ld_(rzn) / np.maximum(ld_(rz), TINY64))
    assert rel_ratio(beta.np(), want) <= 4 * U2 and np.isfinite(beta.np()).all() and abs(beta.np()[1] - 1e5) <= 1e-9


def _case(rng, n=1023, k=100, kp=112, t=11):
    lt, ld = factor(rng, n, k, kp)
    cinv = rng.standard_normal((kp, kp)) / math.sqrt(kp)
    b = dict(n=n, k=k, kp=kp, t=t, ld=ld, LT=Buf(lt, dtype=F32), R=Buf(rng.standard_normal((n, t)), dtype=F64),
             CINV=Buf(0.5 * (cinv + cinv.T), dtype=F64), SC=Buf(np.array([1.0, 0.5]), dtype=F64),
             TM=Buf(rng.standard_normal((kp, 16)), dtype=F64), work=Buf(count=work_doubles(n, kp, t), dtype=F64),
             P=Buf(rng.standard_normal((n, t)), dtype=F64), vec=Buf(rng.uniform(0.5, 2.0, t), dtype=F64),
             ACT=Buf(np.ones(t), dtype=F64))
    return b


def _outputs(b):
    n, kp, t = b["n"], b["kp"], b["t"]
    return dict(G=Buf(count=kp * 16, dtype=F64), T=Buf(count=kp * 16, dtype=F64), Z=Buf(count=n * t, dtype=F64),
                RZ=Buf(count=t, dtype=F64), P=Buf(b["P"].before, dtype=F64), beta=Buf(count=t, dtype=F64),
                act_out=Buf(count=t, dtype=F64))


def _run_all(lib, b, o, s):
    n, k, kp, t, ld = b["n"], b["k"], b["kp"], b["t"], b["ld"]
    nv.check(lib.plx_pcg_gram_f64(b["LT"].ptr, ld, kp, b["R"].ptr, n, t, o["G"].ptr, b["work"].ptr, s), "plx_pcg_gram_f64")
    nv.check(lib.plx_pcg_project_f64(b["LT"].ptr, ld, kp, b["R"].ptr, n, t, b["CINV"].ptr, o["T"].ptr, b["work"].ptr, s),
             "plx_pcg_project_f64")
    nv.check(lib.plx_pcg_apply_f64(b["LT"].ptr, ld, kp, k, b["R"].ptr, n, t, o["T"].ptr, b["SC"].ptr, o["Z"].ptr, o["RZ"].ptr,
                                   b["work"].ptr, s), "plx_pcg_apply_f64")
    nv.check(lib.plx_pcg_step_direction_f64(o["P"].ptr, o["Z"].ptr, o["RZ"].ptr, b["vec"].ptr, b["vec"].ptr, b["ACT"].ptr,
                                            b["vec"].ptr, 1e-3, n, t, o["beta"].ptr, o["act_out"].ptr, s),
             "plx_pcg_step_direction_f64")


def test_graph_replay_equals_eager():
    """The four calls neither allocate nor synchronise: captured into one graph and replayed, they give the eager bits."""
    lib = nv.lib()
    b = _case(np.random.default_rng(7))
    eager, replay = _outputs(b), _outputs(b)
    _run_all(lib, b, eager, stream())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _run_all(lib, b, replay, ctypes.c_void_p(s.cuda_stream))
    graph.replay()
    torch.cuda.synchronize()
    for name in eager:
        assert torch.equal(bits(eager[name].cpu()), bits(replay[name].cpu())), name
        assert replay[name].guards_intact()
    assert not (eager["Z"].cpu() == SENTINEL).any()


def test_refusals_leave_outputs_untouched():
    """Every PLX_ERR_INVALID on device buffers: the sentinel-filled outputs come back untouched, guards intact."""
    lib = nv.lib()
    b = _case(np.random.default_rng(8), n=257, k=17, kp=32, t=4)
    n, k, kp, t, ld = b["n"], b["k"], b["kp"], b["t"], b["ld"]
    o = _outputs(b)
    odd = lambda buf: ctypes.c_void_p(buf.ptr.value + 4)        # noqa: E731
    off8 = ctypes.c_void_p(b["LT"].ptr.value + 8)
    s = stream()

    def gram(lt=b["LT"].ptr, ld=ld, kp=kp, r=b["R"].ptr, n=n, t=t, g=o["G"].ptr, w=b["work"].ptr):
        return lib.plx_pcg_gram_f64(lt, ld, kp, r, n, t, g, w, s)

    def project(lt=b["LT"].ptr, ld=ld, kp=kp, r=b["R"].ptr, n=n, t=t, c=b["CINV"].ptr, tm=o["T"].ptr, w=b["work"].ptr):
        return lib.plx_pcg_project_f64(lt, ld, kp, r, n, t, c, tm, w, s)

    def apply(lt=b["LT"].ptr, ld=ld, kp=kp, k=k, r=b["R"].ptr, n=n, t=t, tm=b["TM"].ptr, sc=b["SC"].ptr, z=o["Z"].ptr,
              rz=o["RZ"].ptr, w=b["work"].ptr):
        return lib.plx_pcg_apply_f64(lt, ld, kp, k, r, n, t, tm, sc, z, rz, w, s)

    def direction(p=o["P"].ptr, z=b["R"].ptr, a=b["vec"].ptr, act=b["ACT"].ptr, n=n, vd=t, beta=o["beta"].ptr,
                  out=o["act_out"].ptr):
        return lib.plx_pcg_step_direction_f64(p, z, a, a, a, act, a, 1e-3, n, vd, beta, out, s)

    shape = (dict(t=0), dict(t=17), dict(n=0), dict(ld=ld - 64), dict(ld=ld + 32), dict(kp=kp + 8), dict(kp=0), dict(kp=1040),
             dict(lt=None), dict(lt=off8), dict(r=None), dict(r=odd(b["R"])), dict(w=None))
    for call, extra in ((gram, (dict(g=None), dict(g=odd(o["G"])))),
                        (project, (dict(c=None), dict(tm=None), dict(tm=odd(o["T"])))),
                        (apply, (dict(k=kp + 1), dict(k=-1), dict(z=b["R"].ptr), dict(tm=None), dict(sc=None), dict(z=None),
                                 dict(rz=odd(o["RZ"])), dict(z=odd(o["Z"]))))):
        for bad in shape + extra:
            assert call(**bad) == PLX_ERR_INVALID, (call.__name__, bad)
    for bad in (dict(vd=0), dict(vd=257), dict(n=0), dict(p=None), dict(z=None), dict(a=None), dict(act=None), dict(beta=None),
                dict(out=None), dict(out=b["ACT"].ptr), dict(p=odd(o["P"]))):
        assert direction(**bad) == PLX_ERR_INVALID, ("direction", bad)
    torch.cuda.synchronize()
    for name in ("G", "T", "Z", "RZ", "beta", "act_out"):
        assert (o[name].cpu() == SENTINEL).all() and o[name].guards_intact(), name
    assert o["P"].unchanged() and o["P"].guards_intact()
    check_buffers(inputs=(b["LT"], b["R"], b["CINV"], b["SC"], b["TM"], b["vec"], b["ACT"]), outputs=(b["work"],))
    assert (b["work"].cpu() == SENTINEL).all()


# ---- the class -----------------------------------------------------------------------------------------------------------
def _double_model(d, kernel="rbf", noise=1.0):
    k = plx.RBFLattice(order=1, ard_num_dims=d) if kernel == "rbf" else plx.MaternLattice(nu=1.5, order=1, ard_num_dims=d)
    model = solvers.LatticeGP(k).double().cuda()
    with torch.no_grad():
        model.raw_noise.fill_(math.log(math.expm1(noise - model.min_noise)))      # noise = softplus(raw) + min_noise
    return model


@pytest.mark.parametrize("kernel", ("rbf", "matern32"))
@pytest.mark.parametrize("d", (3, 8))
def test_class(d, kernel):
    """LatticePreconditioner64 on a Lattice64-sized cloud (n = 701, rank 100, noise 0.1).

    The composed bar of solve(): with Z = (R - L T) / s2 and T = Cinv (L^T R) + dp, Cinv = C^-1 + D,
        P Z - R = -P L (D G + dp) / s2 + P da        (G = L^T R; the exact expression gives 0)
    so |P Z - R| <= |P| (|L| (|D| |G| + |dp|) / s2 + |da|) entry by entry, with |dp| the project bar, |da| the apply bar (on
    |Cinv| |L|^T |R| >= |T|), and every entry of D bounded by its 2-norm: a Cholesky-based inverse of the k x k matrix C has
    ||D||_2 <= (3 k + 1) U2 cond_2(C) ||C^-1||_2 (one backward-stable solve per column)."""
    n, rank, noise = 701, 100, 0.1
    try:
        model = _double_model(d, kernel, noise)
        x = f64t.cuda(cloud("gauss1", n, d, seed=11), np.float64)
        pre = model.preconditioner(x, rank)
        assert type(pre) is solvers.LatticePreconditioner64 and pre.rank == rank and pre.kp == 112
        assert model.preconditioner(x, rank) is pre and model.preconditioner_reuses == 1
        L = pre.L
        assert L.dtype == F64 and tuple(L.shape) == (n, rank)
        assert pre._factor.dtype == F32 and bool((pre._factor[rank:] == 0).all()) and bool((pre._factor[:, n:] == 0).all())
        # the same factor as the fp32 class builds on this lattice: another order and width, the same numbers
        pre32 = solvers.LatticePreconditioner(pre.lat, model.outputscale, model.noise, rank, factor_dtype=F32)
        assert torch.equal(pre32.L.double(), L)
        del pre32
        Ln = ld_(L.cpu().numpy())
        La = np.abs(Ln)
        s2 = LD(pre.noise)
        k = rank
        # C under the gram bar (the noise on the diagonal is one more term)
        C_want = Ln.T @ Ln + s2 * np.eye(k, dtype=LD)
        e = entry_ratio(pre._C.cpu().numpy(), f64_(C_want), f64_(La.T @ La + s2 * np.eye(k, dtype=LD)))
        note("LatticePreconditioner64.C", e, (n + 4) * U2)
        assert e <= (n + 4) * U2, ("C", e)
        # solve: 20 columns = a tile of 16 and one of 4
        P = Ln @ Ln.T + s2 * np.eye(n, dtype=LD)
        R = torch.randn(n, 20, generator=torch.Generator().manual_seed(5), dtype=F64).cuda()
        Z = pre.solve(R)
        assert Z.dtype == F64 and Z.shape == R.shape
        Rn, Zn = ld_(R.cpu().numpy()), ld_(Z.cpu().numpy())
        C64 = f64_(C_want)
        cinv_abs = np.abs(np.linalg.inv(C64))
        dnorm = (3 * k + 1) * U2 * np.linalg.cond(C64) * np.linalg.norm(np.linalg.inv(C64), 2)
        G_abs = f64_(La.T @ np.abs(Rn))                                  # >= |G|
        T_abs = cinv_abs @ G_abs                                         # >= |T| up to rounding
        dp = (n + pre.kp + 8) * U2 * T_abs
        da = (k + 6) * U2 * (np.abs(f64_(Rn)) + f64_(La) @ T_abs) / float(s2)
        bar = f64_(np.abs(P)) @ (f64_(La) @ (dnorm * G_abs.sum(0, keepdims=True) + dp) / float(s2) + da)
        err = np.abs(f64_(P @ Zn - Rn))
        ratio = float((err / bar).max())
        note("LatticePreconditioner64.solve", ratio, 1.0)
        assert ratio <= 1.0, ("solve", ratio)
        with pytest.raises(TypeError, match="float64"):
            pre.solve(R.float())
        # sample: the same draws, in PivotedCholeskyPreconditioner.sample's order
        t = 20
        S = pre.sample(t, generator=torch.Generator(device="cuda").manual_seed(9))
        g = torch.Generator(device="cuda").manual_seed(9)
        g1 = torch.randn(rank, t, generator=g, device="cuda", dtype=F64).cpu().numpy()
        g2 = torch.randn(n, t, generator=g, device="cuda", dtype=F64).cpu().numpy()
        sigma = math.sqrt(pre.noise)
        want = f64_(Ln @ ld_(g1) + LD(sigma) * ld_(g2))
        Ts = np.abs(sigma * g2) + f64_(La) @ np.abs(g1)
        e = entry_ratio(S.cpu().numpy(), want, Ts)
        note("LatticePreconditioner64.sample", e, (k + 6) * U2)
        assert S.dtype == F64 and e <= (k + 6) * U2, ("sample", e)
        # logdet against the dense matrix
        sign, want_ld = np.linalg.slogdet(f64_(P))
        rel = abs(pre.logdet() - want_ld) / abs(want_ld)
        print(f"d={d} {kernel}: logdet {pre.logdet():.15g} against slogdet {want_ld:.15g}: {rel:.2e} relative")
        assert sign == 1.0 and rel <= 1e-12, rel
        # a factor whose lattice has been rebuilt since
        pre.build_id -= 1
        try:
            for call in (lambda: pre.solve(R), lambda: pre.sample(2)):
                with pytest.raises(RuntimeError, match="rebuilt"):
                    call()
        finally:
            pre.build_id += 1
    finally:
        plx.lattice_cache().clear()


# ---- the solve -------------------------------------------------------------------------------------------------------------
def _yardstick():
    n, d = 2000, 3
    x = cloud("gauss1", n, d, seed=1)
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(0), dtype=F64)
    return n, d, x, B


def test_khat_solve_preconditioned():
    """(a), (b) khat_solve of a double LatticeGP(RBFLattice) at noise 1.0 on the yardstick cloud (n = 2000, d = 3) with the
    rank-100 native preconditioner at tol 1e-11: the route is taken (LatticePreconditioner64, the native iteration), the true
    residual through khat_matmul is <= 1e-10, and the native iteration stops within check_every iterations of the torch loop
    (_batched_pcg, NATIVE_PCG_F64 = False) around the same preconditioner.
    Reference on the CPU: numpy PCG in double on s Lattice64.matrix() + noise I (the model's taps, lengthscale and
    outputscale softplus(0)) with P = L L^T + noise I, L the rank-100 float64 pivoted Cholesky factor of s K, reaches a true
    relative residual of 7.4e-12 at iteration 28 (checked every 4), so the bar of 1e-10 stands; no iteration cap below max_iter is set."""
    n, d, x, B = _yardstick()
    check_every = 4
    try:
        model = _double_model(d)
        xt, rhs = f64t.cuda(x, np.float64), B.cuda()
        pre = model.preconditioner(xt, 100)
        assert type(pre) is solvers.LatticePreconditioner64            # (b): fails without the feature
        its = {}
        for native in (True, False):
            called = []
            real = solvers._batched_pcg_native
            solvers._batched_pcg_native = lambda *a, **k: (called.append(1), real(*a, **k))[1]
            solvers.NATIVE_PCG_F64 = native
            try:
                X, info = model.khat_solve(xt, rhs, tol=1e-11, max_iter=1000, precond=pre, check_every=check_every,
                                           want_tridiag=True)
            finally:
                solvers.NATIVE_PCG_F64 = True
                solvers._batched_pcg_native = real
            assert bool(called) == native
            assert X.dtype == F64 and X.shape == rhs.shape and info["rz0"].dtype == F64
            assert tuple(info["tridiag"].shape) == (3, info["iterations"], info["iterations"])
            with torch.no_grad():
                res = float((model.khat_matmul(xt)(X) - rhs).norm() / rhs.norm())
            its[native] = info["iterations"]
            print(f"preconditioned khat_solve in double, native {native}: {info['iterations']} iterations, residual through "
                  f"khat_matmul {res:.2e}")
            assert res <= 1e-10, (native, res)
        assert abs(its[True] - its[False]) <= check_every, its
        # rz0 = B^T P^-1 B
        want = (rhs * pre.solve(rhs)).sum(0)
        assert float(((info["rz0"] - want).abs() / want.abs()).max()) <= 1e-12
        # more than 16 columns keep the torch loop, with the native solve() inside
        wide = torch.randn(n, 17, generator=torch.Generator().manual_seed(1), dtype=F64).cuda()
        Xw, _ = model.khat_solve(xt, wide, tol=1e-11, max_iter=1000, precond=pre)
        with torch.no_grad():
            assert float((model.khat_matmul(xt)(Xw) - wide).norm() / wide.norm()) <= 1e-10
    finally:
        plx.lattice_cache().clear()


def _torch_form(pre):
    """PivotedCholeskyPreconditioner around the native class's own factor (its __init__ without the factorisation loop)."""
    t = object.__new__(solvers.PivotedCholeskyPreconditioner)
    t.Lt, t.noise, t.n, t.rank = pre.L.t().contiguous(), pre.noise, pre.n, pre.rank
    C = t._gram(t.Lt.t()).double() + t.noise * torch.eye(t.rank, dtype=F64, device=t.Lt.device)
    t._chol = torch.linalg.cholesky(C)
    return t


def test_marginal_log_likelihood_preconditioned():
    """(c) marginal_log_likelihood(model.double(), x, y, pre_size=100) and its backward() (n = 600, d = 3, 4 probes, cg_tol
    1e-10): the value and every hyper-parameter gradient agree to 1e-8 relative with the torch loop.  The two factors differ
    (the batched fp32 factor here, the float64 torch factor with NATIVE_PCG_F64 = False: different matrices P, hence
    different probes and a different estimator), so the comparison is against the torch loop (NATIVE_PCG_F64 = False) driven
    with a PivotedCholeskyPreconditioner that holds the native class's own L: the same P, the same draws."""
    n, d = 600, 3
    x = f64t.cuda(cloud("gauss1", n, d, seed=2), np.float64)
    y = torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(3), dtype=F64).cuda()
    values, grads = {}, {}
    try:
        for native in (True, False):
            model = _double_model(d)
            if not native:
                torch_pre = _torch_form(model.preconditioner(x, 100))
                model.preconditioner = lambda *a, **k: torch_pre
            solvers.NATIVE_PCG_F64 = native
            try:
                mll = solvers.marginal_log_likelihood(model, x, y, num_probes=4, cg_tol=1e-10, pre_size=100)
                assert mll.dtype == F64 and bool(torch.isfinite(mll))
                mll.backward()
            finally:
                solvers.NATIVE_PCG_F64 = True
            if native:
                assert type(model.__dict__["_last_preconditioner"]) is solvers.LatticePreconditioner64
            values[native] = float(mll)
            grads[native] = {name: prm.grad.detach().cpu().clone() for name, prm in model.named_parameters()}
            for name, g in grads[native].items():
                assert g.dtype == F64 and bool(torch.isfinite(g).all()), name
            plx.lattice_cache().clear()
    finally:
        plx.lattice_cache().clear()
    diff = abs(values[True] - values[False]) / abs(values[False])
    print(f"preconditioned marginal_log_likelihood in double: native {values[True]:.15g}, torch loop {values[False]:.15g}, "
          f"relative difference {diff:.2e}")
    worst = {}
    for name in grads[True]:
        a, b = grads[True][name], grads[False][name]
        worst[name] = float(((a - b).abs() / b.abs()).max())
        print(f"  grad {name}: native {a.reshape(-1).tolist()}, torch loop {b.reshape(-1).tolist()}, relative {worst[name]:.2e}")
    assert diff <= 1e-8, (values, diff)
    assert all(v <= 1e-8 for v in worst.values()), worst


def test_switch_off_reproduces_the_torch_route():
    """(d) NATIVE_PCG_F64 = False: preconditioner() on a double CUDA x builds PivotedCholeskyPreconditioner, and khat_solve
    with it returns the bits of the expression the torch route has always evaluated."""
    n, d, x, B = _yardstick()
    try:
        model = _double_model(d)
        xt, rhs = f64t.cuda(x[:600], np.float64), B[:600].cuda()
        solvers.NATIVE_PCG_F64 = False
        try:
            pre = model.preconditioner(xt, 20)
            assert type(pre) is solvers.PivotedCholeskyPreconditioner and pre.Lt.dtype == F64
            assert "_last_preconditioner" not in model.__dict__
            X, info = model.khat_solve(xt, rhs, tol=1e-8, max_iter=200, precond=pre)
            with torch.no_grad():
                ref = lk.position_hint(xt.div(model.kernel.lengthscale), xt, scale_of=getattr(model.kernel, "raw_lengthscale", None))
                lat = lk.lattice_cache().get(ref, model.kernel.dkernel_fn.get_coeffs())
                s, noise = model.outputscale, model.noise
                Xp, infop = solvers.batched_cg(lambda V: lat.apply(V).mul_(s).addcmul_(V, noise), rhs, tol=1e-8, max_iter=200,
                                               precond=pre)
        finally:
            solvers.NATIVE_PCG_F64 = True
        assert info["iterations"] == infop["iterations"] and torch.equal(bits(X), bits(Xp))
        assert type(model.preconditioner(xt, 20)) is solvers.LatticePreconditioner64
    finally:
        plx.lattice_cache().clear()


def report():
    lines = ["float64 preconditioner kernels, worst error / derived bar per kernel:"]
    lines += [f"  {k}: {v:.3f}" for k, v in sorted(WORST.items())]
    return "\n".join(lines)


def test_every_new_kernel_was_launched():
    """Every __global__ kernel of plx_pcg_f64.hip, every column count of the apply pass and the three kernels of
    plx_cg_kernels.h that this file's entry points launch (the final sum of <R, Z>, the two direction forms) ran in this
    module (run as a whole), under its bar."""
    print(report())
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplex_gp_amd", "csrc")
    find = r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\("
    kernels = set(re.findall(find, re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "plx_pcg_f64.hip")).read())))
    assert kernels == {"pcg64_gram_kernel", "pcg64_project_kernel", "pcg64_apply_kernel"}, kernels
    shared = {"coldot_final_kernel", "step_direction_kernel", "step_direction_vec_kernel"}
    assert shared <= set(re.findall(find, re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "plx_cg_kernels.h")).read())))
    reached = {k.split("<")[0] for k in REACHED}
    assert kernels | shared <= reached, sorted((kernels | shared) - reached)
    assert {f"pcg64_apply_kernel<{t}>" for t in TS} <= REACHED
    assert all(v <= 1.0 for v in WORST.values()), WORST
