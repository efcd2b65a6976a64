"""The float64 conjugate-gradient solve (simplex_gp_amd/csrc/plx_cg_f64.hip) on the GPU: the three vector calls, the affine
product plx_apply_affine_f64, and the solve through solvers.batched_cg, LatticeGP.khat_solve and marginal_log_likelihood.

Bars are derived, never measured.  With U2 = 2^-52 (the unit roundoff 2^-53 once for each side of a comparison) and T the
sum of the absolute values of the terms an entry adds up (tests/solver64.coldot64 / axpy64 return it):
  * a column sum of n terms: (n + 4) U2 T.  n - 1 additions in ANY order give at most (n - 1) u T to first order, the
    products one more u each, the reference its own; the bound holds for every summation tree, so the kernel's is not
    restated here;
  * an axpy entry y + a x: 4 U2 T (one product, one sum -- or one fma -- per side);
  * a coefficient rs / pAp: 4 U2 relative to the double inputs it was formed from (one division per side);
  * the affine product against a * Lattice64 + b * I: the bar of tests/test_f64_gpu.py, k U2 of T with k raised by 2 (the
    product with b and the fma), T = |a| terms64(v) + |b v|.
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
from simplex_gp_amd import solvers
from simplex_gp_amd._native import PlxError
from tests.gpubuf import SENTINEL, Buf, check_buffers
from tests.lattice64 import Lattice64, cloud
from tests.solver64 import active64, axpy64, coldot64, entry_ratio, rel_ratio

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -52
TINY64 = 1e-300
PLX_ERR_INVALID, PLX_ERR_STATE = 1, 5
F64 = torch.float64
LD = np.longdouble

NS = (1, 255, 257, 1023, 3077)           # fewer rows than workgroups, a ragged last step, several rows per lane
VDS = (1, 2, 3, 4, 11, 12, 16, 101, 255, 256)

WORST = {}                               # kernel -> worst error / bar
REACHED = set()


def note(kernel, ratio, bar):
    REACHED.add(kernel)
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio / bar)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def colsum_ld(a, b):
    """(sum_r a b in longdouble, rounded to double; T = sum_r |a b|) per column."""
    p = np.asarray(a, LD) * np.asarray(b, LD)
    return np.asarray(p.sum(0), np.float64), coldot64(a, b)[1]


def axpy_ld(y, a, x):
    want = np.asarray(y, LD) + np.asarray(a, LD) * np.asarray(x, LD)
    return np.asarray(want, np.float64), axpy64(y, a, x)[1]


def direction_kernel(n, vd, off):
    """plx_cg_step_direction_f64: two elements per thread when n vd is even and both matrices are 16-byte aligned."""
    return "step_direction_vec_kernel" if (n * vd) % 2 == 0 and off % 2 == 0 else "step_direction_kernel"


def work_doubles(vd):
    return int(nv.lib().plx_coldot_work_doubles(vd))


def scalars(rng, vd, n, scale=1.0):
    """rs, pAp, b_norm of a plausible iteration: positive, a few orders of magnitude apart."""
    rs = rng.uniform(0.5, 2.0, vd) * n * scale ** 2
    pap = rng.uniform(0.5, 2.0, vd) * n * scale ** 2
    return rs, pap


@pytest.mark.parametrize("vd", VDS)
@pytest.mark.parametrize("n", NS)
def test_vector_kernels(n, vd):
    """plx_coldot_f64, plx_cg_step_update_f64 and plx_cg_step_direction_f64 at one shape, buffers aligned and offset by one
    double: against longdouble under the derived bars; one column inactive; two calls bit-equal; guards intact."""
    lib = nv.lib()
    rng = np.random.default_rng(1000 * n + vd)
    inactive = vd // 2 if vd > 1 else None
    for off in (0, 1):
        label = f"n={n} vd={vd} off={off}"
        a, b = rng.standard_normal((n, vd)), rng.standard_normal((n, vd))
        # ---- coldot
        A, B_ = Buf(a, offset=off, dtype=F64), Buf(b, offset=off, dtype=F64)
        out, work = Buf(count=vd, offset=off, dtype=F64), Buf(count=work_doubles(vd), offset=off, dtype=F64)
        nv.check(lib.plx_coldot_f64(A.ptr, B_.ptr, n, vd, out.ptr, work.ptr, stream()), "plx_coldot_f64")
        want, T = colsum_ld(a, b)
        e = entry_ratio(out.np(), want, T)
        note("coldot_partial_kernel", e, (n + 4) * U2)
        REACHED.add("coldot_final_kernel")
        assert e <= (n + 4) * U2, (label, "coldot", e)
        first = out.cpu().clone()
        nv.check(lib.plx_coldot_f64(A.ptr, B_.ptr, n, vd, out.ptr, work.ptr, stream()), "plx_coldot_f64")
        assert torch.equal(out.cpu().view(torch.int64), first.view(torch.int64)), (label, "coldot not deterministic")
        check_buffers(inputs=(A, B_), outputs=(out, work))
        # ---- step_update
        x0, r0, p0, ap0 = (rng.standard_normal((n, vd)) for _ in range(4))
        rs, pap = scalars(rng, vd, n)
        act = np.ones(vd)
        if inactive is not None:
            act[inactive] = 0.0
        results = []
        for _ in range(2):
            X, R = Buf(x0, offset=off, dtype=F64), Buf(r0, offset=off, dtype=F64)
            P, AP = Buf(p0, offset=off, dtype=F64), Buf(ap0, offset=off, dtype=F64)
            RS, PAP, ACT = Buf(rs, dtype=F64), Buf(pap, dtype=F64), Buf(act, dtype=F64)
            rs_new, alpha = Buf(count=vd, offset=off, dtype=F64), Buf(count=vd, offset=off, dtype=F64)
            nv.check(lib.plx_cg_step_update_f64(X.ptr, R.ptr, P.ptr, AP.ptr, RS.ptr, PAP.ptr, ACT.ptr, n, vd, rs_new.ptr,
                                                alpha.ptr, work.ptr, stream()), "plx_cg_step_update_f64")
            check_buffers(inputs=(P, AP, RS, PAP, ACT), outputs=(X, R, rs_new, alpha, work))
            results.append((X.cpu(), R.cpu(), rs_new.cpu(), alpha.cpu()))
        for u, v in zip(*results):
            assert torch.equal(u.view(torch.int64), v.view(torch.int64)), (label, "step_update not deterministic")
        gx, gr, grs, ga = (t.numpy() for t in results[0])
        gx, gr = gx.reshape(n, vd), gr.reshape(n, vd)
        alpha_want = np.where(act > 0, np.asarray(np.asarray(rs, LD) / np.maximum(np.asarray(pap, LD), TINY64), np.float64), 0.0)
        ea = rel_ratio(ga, alpha_want)
        note("cg_update_kernel", ea, 4 * U2)
        assert ea <= 4 * U2, (label, "alpha", ea)
        wx, Tx = axpy_ld(x0, ga, p0)                         # from the alpha the kernel formed
        wr, Tr = axpy_ld(r0, -ga, ap0)
        ex, er = entry_ratio(gx, wx, Tx), entry_ratio(gr, wr, Tr)
        note("cg_update_kernel", max(ex, er), 4 * U2)
        assert ex <= 4 * U2 and er <= 4 * U2, (label, "X / R", ex, er)
        wrs, Trs = colsum_ld(gr, gr)                         # |R|^2 of the R the kernel stored
        ers = entry_ratio(grs, wrs, Trs)
        note("cg_update_kernel", ers, (n + 4) * U2)
        assert ers <= (n + 4) * U2, (label, "rs_new", ers)
        if inactive is not None:
            assert ga[inactive] == 0.0
            assert np.array_equal(gx[:, inactive].view(np.int64), x0[:, inactive].view(np.int64)), (label, "X of a frozen column")
            assert np.array_equal(gr[:, inactive].view(np.int64), r0[:, inactive].view(np.int64)), (label, "R of a frozen column")
        # ---- step_direction (tol far from every column's sqrt(rs_new) / b_norm)
        b_norm = np.sqrt(rs) * rng.uniform(10.0, 20.0, vd)
        tol = 1e-3
        results = []
        for _ in range(2):
            P, R = Buf(p0, offset=off, dtype=F64), Buf(gr, offset=off, dtype=F64)
            RSN, RS, ACT, BN = Buf(grs, dtype=F64), Buf(rs, dtype=F64), Buf(act, dtype=F64), Buf(b_norm, dtype=F64)
            beta, act_out = Buf(count=vd, offset=off, dtype=F64), Buf(count=vd, offset=off, dtype=F64)
            nv.check(lib.plx_cg_step_direction_f64(P.ptr, R.ptr, RSN.ptr, RS.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr,
                                                   act_out.ptr, stream()), "plx_cg_step_direction_f64")
            check_buffers(inputs=(R, RSN, RS, ACT, BN), outputs=(P, beta, act_out))
            results.append((P.cpu(), beta.cpu(), act_out.cpu()))
        for u, v in zip(*results):
            assert torch.equal(u.view(torch.int64), v.view(torch.int64)), (label, "step_direction not deterministic")
        gp, gb, gact = (t.numpy() for t in results[0])
        kernel = direction_kernel(n, vd, off)
        beta_want = np.where(act > 0, np.asarray(np.asarray(grs, LD) / np.maximum(np.asarray(rs, LD), TINY64), np.float64), 0.0)
        eb = rel_ratio(gb, beta_want)
        wp, Tp = axpy_ld(gr, gb, p0)
        ep = entry_ratio(gp.reshape(n, vd), wp, Tp)
        note(kernel, max(eb, ep), 4 * U2)
        assert eb <= 4 * U2 and ep <= 4 * U2, (label, kernel, eb, ep)
        flag, decided = active64(act, grs, b_norm, tol)
        assert decided.all() and np.array_equal(gact, flag.astype(np.float64)), (label, "active_out", gact, flag)
        if inactive is not None:
            assert gb[inactive] == 0.0 and gact[inactive] == 0.0


@pytest.mark.parametrize("vd", (3, 12))
def test_threshold_and_small_scale(vd):
    """A column's rs_new on either side of tol * b_norm by a margin of 1e-3 decides its flag; and the 1e-300 guard: the
    iteration of a right-hand side scaled by 1e-20 (rs, pAp near 1e-40 n) forms the alpha of the unscaled one."""
    lib = nv.lib()
    n = 257
    rng = np.random.default_rng(vd)
    tol = 1e-6
    rs, _ = scalars(rng, vd, n)
    b_norm = rng.uniform(1.0, 2.0, vd)
    side = np.where(np.arange(vd) % 2 == 0, 1.0 + 2e-3, 1.0 - 2e-3)
    rs_new = (tol * b_norm * side) ** 2
    act = np.ones(vd)
    p0, r0 = rng.standard_normal((n, vd)), rng.standard_normal((n, vd))
    P, R = Buf(p0, dtype=F64), Buf(r0, dtype=F64)
    RSN, RS, ACT, BN = Buf(rs_new, dtype=F64), Buf(rs, dtype=F64), Buf(act, dtype=F64), Buf(b_norm, dtype=F64)
    beta, act_out = Buf(count=vd, dtype=F64), Buf(count=vd, dtype=F64)
    nv.check(lib.plx_cg_step_direction_f64(P.ptr, R.ptr, RSN.ptr, RS.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr, act_out.ptr,
                                           stream()), "plx_cg_step_direction_f64")
    flag, decided = active64(act, rs_new, b_norm, tol, margin=1e-3)
    assert decided.all(), "the margin of 2e-3 in sqrt(rs_new) is outside active64's 1e-3"
    assert np.array_equal(act_out.np(), flag.astype(np.float64)) and set(flag.tolist()) == {0.0, 1.0}
    # ---- the same update at scale 1 and at scale 1e-20
    x0, ap0 = rng.standard_normal((n, vd)), rng.standard_normal((n, vd))
    rs, pap = scalars(rng, vd, n)
    alphas = {}
    for scale in (1.0, 1e-20):
        X, R = Buf(x0 * scale, dtype=F64), Buf(r0 * scale, dtype=F64)
        P, AP = Buf(p0 * scale, dtype=F64), Buf(ap0 * scale, dtype=F64)
        RS, PAP = Buf(rs * scale * scale, dtype=F64), Buf(pap * scale * scale, dtype=F64)
        rsn, alpha, work = Buf(count=vd, dtype=F64), Buf(count=vd, dtype=F64), Buf(count=work_doubles(vd), dtype=F64)
        nv.check(lib.plx_cg_step_update_f64(X.ptr, R.ptr, P.ptr, AP.ptr, RS.ptr, PAP.ptr, ACT.ptr, n, vd, rsn.ptr, alpha.ptr,
                                            work.ptr, stream()), "plx_cg_step_update_f64")
        fed = np.asarray(np.asarray(RS.np(), LD) / np.maximum(np.asarray(PAP.np(), LD), TINY64), np.float64)
        e = rel_ratio(alpha.np(), fed)
        print(f"vd={vd} scale={scale:g}: alpha against rs / pAp of its own inputs: {e:.2e} (bar {4 * U2:.2e}); pAp ~ {PAP.np()[0]:.1e}")
        assert e <= 4 * U2, (scale, e)
        alphas[scale] = alpha.np()
        wrs, Trs = colsum_ld(R.np(n, vd), R.np(n, vd))
        assert entry_ratio(rsn.np(), wrs, Trs) <= (n + 4) * U2
    assert float(PAP.np().max()) < 1e-30, "the scaled pAp must lie below the fp32 calls' guard for this to test anything"
    e = rel_ratio(alphas[1e-20], alphas[1.0])
    print(f"vd={vd}: alpha at scale 1e-20 against alpha at scale 1: {e:.2e} (bar {4 * U2:.2e})")
    assert e <= 4 * U2, e


# ---- plx_apply_affine_f64 --------------------------------------------------------------------------------------------------
AFF_V1, AFF_CHUNK, AFF_WIDE = "f64_affine_v1_kernel", "f64_affine_chunk_kernel", "f64_affine_wide_kernel"
AFF_VDS = (1, 2, 3, 11, 12, 101, 128, 129, 520)


def affine_expect(vd):
    nch = (vd + 1) // 2
    return AFF_V1 if vd == 1 else AFF_CHUNK if nch <= 64 else AFF_WIDE


def _affine_cases():
    out = [("d8", vd, i % 2 == 0) for i, vd in enumerate(AFF_VDS)]        # every width at one lattice (d + 1 = 9, order 3)
    out += [("d8", 12, False), ("d8", 2, False), ("d8", 1, False)]
    for i, lname in enumerate(("d1", "d3", "d18", "coarse-o0")):          # d in {1, 3, 18}, orders 1, 2, 1, 0
        for j in range(3):
            vd = AFF_VDS[(3 * i + j) % len(AFF_VDS)]
            out.append((lname, vd, (i + j) % 2 == 1))
    out += [("d24", 1, True), ("d24", 12, False)]                         # d + 1 > 20: the run-time form of the slices
    return out


AFF_CASES = _affine_cases()


def raw_affine(lat, src, out, ss, dot=None, work=None, s=None):
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    return nv.lib().plx_apply_affine_f64(lat._h, vp(src), src.shape[1], vp(out), vp(ss), vp(dot), vp(work),
                                         stream() if s is None else s)


@pytest.mark.parametrize("lname,vd,aligned", AFF_CASES, ids=[f"{a}-vd{b}-{'al' if c else 'off'}" for a, b, c in AFF_CASES])
def test_apply_affine_f64(lname, vd, aligned):
    x, l64, taps = f64t.operator(lname)
    n = l64.n
    lat = f64t.gpu_lattice(lname)
    label = f"{lname} vd={vd} {'aligned' if aligned else 'offset'}"
    v = np.random.default_rng(vd + 17).standard_normal((n, vd))
    src = f64t.placed(n, vd, aligned, f64t.cuda(v, np.float64))
    a, b = 0.75, 1.3
    ss = torch.tensor([a, b], dtype=F64, device="cuda")
    one_zero = torch.tensor([1.0, 0.0], dtype=F64, device="cuda")
    # contract (i): (1, 0) gives the values of apply
    plain = lat.apply(src, out=f64t.placed(n, vd, aligned)).clone()
    same = lat.apply_affine(src, one_zero, out=f64t.placed(n, vd, aligned))
    assert lat.f64_kernels()["slice"] == [affine_expect(vd)], (label, lat.f64_kernels())
    REACHED.add(affine_expect(vd))
    assert torch.equal(same, plain), (label, "apply_affine at (1, 0) differs from apply")
    # against a * Lattice64 + b * I in longdouble
    got = lat.apply_affine(src, ss, out=f64t.placed(n, vd, aligned)).clone()
    bytes1 = lat.device_bytes
    want = np.asarray(LD(a) * np.asarray(l64.apply_staged(v), LD) + LD(b) * np.asarray(v, LD), np.float64)
    T = abs(a) * l64.terms64(v) + abs(b) * np.abs(v)
    k = f64t.depth(lat, extra=2)
    e = entry_ratio(got.cpu().numpy(), want, T)
    note(affine_expect(vd), e, k * U2)
    print(f"{label}: k = {k}  entry {e:.2e} (bar {k * U2:.2e})  {affine_expect(vd)}")
    assert e <= k * U2, (label, e, k * U2)
    dot_ok = lat.affine_dot_f64_ok(vd)
    assert dot_ok == (vd <= 128), (label, dot_ok)
    if not dot_ok:
        with pytest.raises(ValueError):
            lat.apply_affine(src, ss, want_dot=True)
        assert lat.device_bytes == bytes1
        return
    # the fused dot: against the longdouble dot of src and the returned out, and contract (ii) against plx_coldot_f64
    got2, dot = lat.apply_affine(src, ss, out=f64t.placed(n, vd, aligned), want_dot=True)
    assert lat.device_bytes == bytes1, (label, "the second call of a width moved plx_device_bytes")
    assert torch.equal(got2, got), (label, "want_dot changed the product")
    assert dot.shape == (vd,) and dot.dtype == F64
    g = got.cpu().numpy()
    wdot, Tdot = colsum_ld(v, g)
    ed = entry_ratio(dot.cpu().numpy(), wdot, Tdot)
    cold = solvers._colsum(src, got)
    eii = entry_ratio(dot.cpu().numpy(), cold.cpu().numpy(), Tdot)
    note(affine_expect(vd) + "/dot", max(ed, eii), (n + 4) * U2)
    print(f"{label}: fused dot against longdouble {ed:.2e}, against plx_coldot_f64 {eii:.2e} (bar {(n + 4) * U2:.2e})")
    assert ed <= (n + 4) * U2 and eii <= (n + 4) * U2, (label, ed, eii)
    _, dot_again = lat.apply_affine(src, ss, want_dot=True)
    assert torch.equal(dot_again.view(torch.int64), dot.view(torch.int64)), (label, "fused dot not deterministic")
    with pytest.raises(ValueError, match="partial"):
        lat.apply_affine(src, ss, want_dot="partial")


def test_apply_affine_refusals():
    """Each refusal with a sentinel-filled out that must come back untouched."""
    rng = np.random.default_rng(5)
    n, d = 3000, 3
    taps = f64t.gauss_taps(1)
    x = f64t.cuda(rng.standard_normal((n, d)))
    ss = torch.tensor([2.0, 0.5], dtype=F64, device="cuda")
    lat = plx.Lattice().build(x, taps)
    sentinel = lambda rows, vd: torch.full((rows, vd), SENTINEL, dtype=F64, device="cuda")      # noqa: E731
    untouched = lambda t: bool((t == SENTINEL).all())                                           # noqa: E731
    # out aliasing src
    v = f64t.cuda(rng.standard_normal((n, 2)), np.float64)
    keep = v.clone()
    assert raw_affine(lat, v, v, ss) == PLX_ERR_INVALID and b"alias" in nv.lib().plx_last_error()
    assert torch.equal(v, keep)
    # d_dot at a width the fused dot does not serve
    v129 = f64t.cuda(rng.standard_normal((n, 129)), np.float64)
    out = sentinel(n, 129)
    dot = sentinel(1, 129)
    work = torch.empty(1 << 16, dtype=F64, device="cuda")
    assert nv.lib().plx_affine_dot_work_doubles(lat._h, 129) == -1 and nv.lib().plx_affine_dot_work_doubles(lat._h, 128) > 0
    assert raw_affine(lat, v129, out, ss, dot, work) == PLX_ERR_INVALID and b"plx_coldot_f64" in nv.lib().plx_last_error()
    assert untouched(out) and untouched(dot)
    # d_dot without d_work
    out2 = sentinel(n, 2)
    assert raw_affine(lat, v, out2, ss, dot, None) == PLX_ERR_INVALID and untouched(out2)
    assert torch.isfinite(lat.apply_affine(v129, ss)).all()                   # without the dot the wide shape serves it
    lat.close()
    # one shard of two
    lat = plx.Lattice().build(x, taps, shard=(0, 2))
    own = v[:lat.n_owned].contiguous()
    out = sentinel(lat.n_owned, 2)
    with pytest.raises(PlxError) as err:
        lat.apply_affine(own, ss, out=out)
    assert err.value.code == PLX_ERR_STATE and "shard" in str(err.value) and untouched(out)
    assert nv.lib().plx_affine_dot_work_doubles(plx.Lattice()._h, 2) == -1   # not built
    lat.close()
    # a stream capture that would have to allocate the float64 workspace
    lat = plx.Lattice().build(x, taps)
    lat.apply(v.float())
    before = lat.device_bytes
    out = sentinel(n, 2)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(PlxError, match="captured") as err:
        with torch.cuda.graph(graph, stream=s):
            lat.apply_affine(v, ss, out=out)
    assert err.value.code == PLX_ERR_STATE and lat.device_bytes == before
    del graph
    torch.cuda.synchronize()
    assert untouched(out)
    # ... and the steady state: no allocation from the second call on, a captured call replays to the same bits
    with torch.cuda.stream(s):
        eager, dot = lat.apply_affine(v, ss, out=out, want_dot=True)
        eager, dot = eager.clone(), dot.clone()
        first = lat.device_bytes
        lat.apply_affine(v, ss, out=out, want_dot=True)
        assert lat.device_bytes == first
        s.synchronize()
        dot_out = torch.zeros(2, dtype=F64, device="cuda")
        work = lat._dot_work64
        graph = torch.cuda.CUDAGraph()
        out.zero_()
        with torch.cuda.graph(graph, stream=s):
            nv.check(raw_affine(lat, v, out, ss, dot_out, work, s=ctypes.c_void_p(s.cuda_stream)), "plx_apply_affine_f64")
        graph.replay()
        s.synchronize()
        assert torch.equal(out, eager) and torch.equal(dot_out.view(torch.int64), dot.view(torch.int64))
        assert lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


# ---- the solve ---------------------------------------------------------------------------------------------------------
def _yardstick():
    n, d = 2000, 3
    taps = np.array([0.5, 1.0, 0.5], np.float32)
    x = cloud("gauss1", n, d, seed=1)
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(0), dtype=F64)
    return n, d, taps, x, B


def test_solve_with_fused_dot():
    """(a) The yardstick solve of DESIGN.md section 14, (K + 1.0 I) X = B at tol 1e-11, by batched_cg with matmul_dot from
    apply_affine: the true residual against the Lattice64 matrix on the CPU is <= 1e-10 (the matrix alone reaches 8.9e-12 in
    168 iterations there), and the native double iteration and the torch loop stop within check_every iterations of each
    other."""
    n, d, taps, x, B = _yardstick()
    K = Lattice64(x, taps).matrix()
    lat = plx.Lattice().build(f64t.cuda(x), taps)
    ss = torch.tensor([1.0, 1.0], dtype=F64, device="cuda")
    rhs = B.cuda()
    check_every = 4
    its = {}
    for native in (True, False):
        solvers.NATIVE_CG_F64 = native
        try:
            X, info = solvers.batched_cg(lambda V: lat.apply_affine(V, ss), rhs, max_iter=1000, tol=1e-11, check_every=check_every,
                                         matmul_dot=lambda V: lat.apply_affine(V, ss, want_dot=True))
        finally:
            solvers.NATIVE_CG_F64 = True
        assert X.dtype == F64
        res = f64t.true_residual(K, X.cpu().numpy(), B.numpy())
        its[native] = info["iterations"]
        print(f"solve (K + I) X = B in double, native iteration {native}: {info['iterations']} iterations, true relative "
              f"residual {res:.2e}")
        assert res <= 1e-10, (native, res)
    assert abs(its[True] - its[False]) <= check_every, its
    REACHED.update(("cg_update_kernel", "coldot_partial_kernel", "coldot_final_kernel"))
    lat.close()


def _double_model(d):
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).double().cuda()
    with torch.no_grad():
        model.raw_noise.fill_(math.log(math.expm1(1.0 - model.min_noise)))      # noise = softplus(raw) + min_noise = 1.0
    return model


def test_khat_solve_in_double():
    """(b) LatticeGP(RBFLattice) in double on the yardstick cloud, noise 1.0: khat_solve(x, rhs, tol=1e-11) returns float64
    and its residual, recomputed with khat_matmul in double, is <= 1e-10.  (numpy CG on s Lattice64.matrix() + noise I for
    the model's own taps -- [0.346, 1, 0.346], lengthscale and outputscale softplus(0) -- reaches a true residual of 1.5e-11
    at iteration 80 on the CPU, so the noise of 1.0 stands.)  On a model without the double solve this raises TypeError."""
    n, d, _, x, B = _yardstick()
    try:
        model = _double_model(d)
        xt, rhs = f64t.cuda(x, np.float64), B.cuda()
        assert abs(float(model.noise) - 1.0) < 1e-12
        X, info = model.khat_solve(xt, rhs, tol=1e-11, max_iter=1000)
        assert X.dtype == F64 and X.shape == rhs.shape
        with torch.no_grad():
            res = float((model.khat_matmul(xt)(X) - rhs).norm() / rhs.norm())
        print(f"khat_solve in double: {info['iterations']} iterations, residual through khat_matmul {res:.2e}")
        assert res <= 1e-10, res
        with model.khat_in_lattice_rows(xt) as (mm, to_rows, from_rows):
            V = rhs[:, :2].contiguous()
            assert to_rows(V) is V and from_rows(V) is V
            got = mm(V)
            assert got.dtype == F64 and float((got - model.khat_matmul(xt)(V)).norm() / got.norm()) <= 1e-14
    finally:
        plx.lattice_cache().clear()


def test_marginal_log_likelihood_in_double():
    """(c) marginal_log_likelihood of a double model (n = 600, d = 3, 4 probes, cg_tol 1e-10, no preconditioner): finite,
    backward() fills every hyper-parameter's .grad in float64, and the value agrees to 1e-8 relative with the same call on
    the torch loop (both solves converge to 1e-10; the SLQ term from slightly different coefficients is the loose part)."""
    n, d = 600, 3
    x = f64t.cuda(cloud("gauss1", n, d, seed=2), np.float64)
    y = torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(3), dtype=F64).cuda()
    values = {}
    try:
        for native in (True, False):
            model = _double_model(d)
            solvers.NATIVE_CG_F64 = native
            try:
                mll = solvers.marginal_log_likelihood(model, x, y, num_probes=4, cg_tol=1e-10, pre_size=0)
                assert mll.dtype == F64 and bool(torch.isfinite(mll))
                mll.backward()
            finally:
                solvers.NATIVE_CG_F64 = True
            for name, prm in model.named_parameters():
                assert prm.grad is not None and prm.grad.dtype == F64 and bool(torch.isfinite(prm.grad).all()), name
            values[native] = float(mll)
            plx.lattice_cache().clear()
    finally:
        plx.lattice_cache().clear()
    diff = abs(values[True] - values[False]) / abs(values[False])
    print(f"marginal_log_likelihood in double: native {values[True]:.15g}, torch loop {values[False]:.15g}, relative "
          f"difference {diff:.2e}")
    assert diff <= 1e-8, (values, diff)


def report():
    lines = ["float64 CG kernels, worst error / derived bar per kernel:"]
    lines += [f"  {k}: {v:.3f}" for k, v in sorted(WORST.items())]
    return "\n".join(lines)


def test_every_new_kernel_was_launched():
    """Every __global__ kernel of plx_cg_f64.hip and of plx_cg_kernels.h, the templated vector steps it instantiates for
    double, ran in this module (run as a whole), and the slice names it reports are the three the affine cases expect."""
    print(report())
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplex_gp_amd", "csrc")
    text = "".join(open(os.path.join(csrc, src)).read() for src in ("plx_cg_f64.hip", "plx_cg_kernels.h"))
    text = re.sub(r"//[^\n]*", "", text)
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\(", text))
    literals = set()
    for stmt in re.finditer(r"\bkn_f64_slice\s*=([^;]*);", text):
        literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    assert literals == {AFF_V1, AFF_CHUNK, AFF_WIDE}, literals
    assert kernels == {"coldot_partial_kernel", "coldot_final_kernel", "cg_update_kernel",
                       "step_direction_kernel", "step_direction_vec_kernel", AFF_V1, AFF_CHUNK, AFF_WIDE}, kernels
    assert kernels <= REACHED, sorted(kernels - REACHED)
    assert all(v <= 1.0 for v in WORST.values()), WORST
