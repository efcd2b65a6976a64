"""The position gradient of a query on the GPU: plx_slice_at_dots / plx_slice_at_dots_f64 (plx_query_kernels.h),
plx_locate_pullback / plx_locate_pullback_f64 (locate_pullback_kernel, plx_build.hip), query_grad.slice_at_dots /
locate_pullback / slice_at_backward, lattice_kernel.LatticeSliceAt and PredictionCache.predict_query_grad.

Yardstick: tests/query_grad64.QueryGrad64 on tests/query64.Query64 (tests/test_query_grad64.py pins it on the CPU).  The
lattices and the query sets are those of tests/test_query_gpu.py.

Bars, derived, not measured (eps = 2^-24 or 2^-52, denom = 1 + 2^-d):
  dots        |t_r - <g, values_r> / denom| <= (vd + 3) eps T_r,  T_r = <|g|, |values_r|> / denom, on the device's own values:
              a sum of vd products in any order is within gamma_vd of the sum of their sizes (one rounding per product,
              at most vd - 1 per addition chain; fused multiply-adds only remove roundings), the rounded reciprocal and the
              multiplication by it (fp32) or the division (double) add two more: vd + 2, one spare.  Exactly 0 where the
              corner is absent.
  pull-back   |gx_j - closed form| <= (d + 6) eps M_j,  M_j = s_j (sum_{i <= j} |e|_i + (j + 1) |e|_{j+1}) formed from |t|.
              Recount: u_k = t_a - t_b is one rounding, e_i = u / (d + 1) a second (the selects are exact), so every e
              carries two; the running sum over i <= j adds at most j more to a term (e_0 enters exactly), the product
              (j + 1) e_{j+1} one (j + 1 converts exactly), the subtraction one, the product with s_j (exact in either
              type) one: a prefix term meets at most j + 4 <= d + 3 roundings, the other term 5.  max(d + 3, 5) <= d + 4,
              so the issue's d + 6 holds with two to spare and is what is asserted.
  end to end  the two composed: (d + 6) eps M(|t| + (vd + 3) eps T) + (vd + 3) eps M(T), M being monotone in its argument;
              plus the reference's own error, which matters in double only: grad64 contracts t with the geometric Jacobian,
              a float64 linear solve, so twice sum_r |t_r| |J_geo - J_closed| (how far the two derivations of the yardstick are
              apart on this very query) and 2^-52 sum_r ((d + 1) |t_r| + vd T_r) |J_geo| for the two float64 sums.
  linearity   the bar of tests/test_query_grad64.py (the reference's own fp32 weight error c: the device's weights are the
              reference's, bit for bit -- tests/test_query_gpu.py, contract 1) plus the end-to-end bar in double.
  prediction  see test_predict_query_grad.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import lattice_kernel, query_grad, training
from tests.lattice64 import cloud
from tests.query64 import Query64
from tests.query_grad64 import U24, QueryGrad64, end_to_end_bar, reference_error, shifted, weight_error, weight_error_cap
from tests.test_f64_gpu import depth
from tests.test_forward_fp64 import ENTRY
from tests.test_query_gpu import (CASES, EPS, F32, F64, IDS, PLX_ERR_INVALID, PLX_ERR_STATE, SLICE_CASES, VDS, _model, _ptr,
                                  cuda, gpu_lattice, id_map, operator, queries, reference)

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -52
NP = {F32: np.float32, F64: np.float64}
WORST = {}
_GRADS = {}


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


def grad_ref(key, name):
    if (key, name) not in _GRADS:
        _GRADS[key, name] = QueryGrad64(reference(key, name), operator(key)[1])
    return _GRADS[key, name]


def expect(vd, dtype):
    """The family: by the row width alone (chunks of 16 bytes), the thresholds of slice_at."""
    nch = (vd + 3) // 4 if dtype == F32 else (vd + 1) // 2
    return "slice_at_dots_v1_kernel" if vd == 1 else "slice_at_dots_chunk_kernel" if nch <= 64 else "slice_at_dots_wide_kernel"


def share(got, want, bar):
    """max |got - want| / bar; inf unless got is exactly `want` wherever the bar is 0, and finite everywhere."""
    got, want, bar = (np.asarray(a, np.float64) for a in (got, want, bar))
    err, zero = np.abs(got - want), bar == 0
    if np.any(err[zero] != 0) or not np.all(np.isfinite(got)):
        return float("inf")
    return float((err[~zero] / bar[~zero]).max()) if np.any(~zero) else 0.0


def blurred(lat, n, vd, dtype, seed):
    """(values on the device, the same as float64 [m, vd])."""
    src = np.random.default_rng(seed).standard_normal((n, vd))
    values, _ = lat.blurred(cuda(src, NP[dtype]))
    return values, values[:lat.m, :vd].cpu().numpy().astype(np.float64)


DOT_CASES = [("gauss1", 1, 3, True, None), ("gauss1", 3, 3, False, None), ("dup", 8, 0, False, None),
             ("gauss1", 8, 2, False, None), ("gauss1", 18, 3, False, 300)]
DOT_IDS = [IDS[CASES.index(k)] for k in DOT_CASES]


# ---- 1: the corner dots ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", DOT_CASES, ids=DOT_IDS)
def test_dots_every_entry(key):
    """Fails without the feature.  Every family, both precisions, an aligned and an unaligned upstream gradient; at the
    `train` queries the dots are also held against the build's own corner table of those points (ARRAY_ENTRY_VERTEX through
    the point permutation): the corner order is the build's."""
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    n = x.shape[0]
    families = set()
    evid = lat.export(nv.ARRAY_ENTRY_VERTEX).astype(np.int64)                      # [d+1, n] in lattice order
    inv = np.empty(n, np.int64)
    inv[lat.export(nv.ARRAY_POINT_PERM).astype(np.int64)] = np.arange(n)
    for vd in VDS:
        for dtype in (F32, F64):
            values, v64 = blurred(lat, n, vd, dtype, 5 + vd)
            bar_k = (vd + 3) * EPS[dtype]
            for name in ("train", "jit", "far"):
                G = grad_ref(key, name)
                Q = queries(key, name)
                q = lat.locate(cuda(Q))
                g = np.random.default_rng(17 + vd).standard_normal((q.nq, vd)).astype(NP[dtype])
                t = query_grad.slice_at_dots(lat, values, q, cuda(g, NP[dtype]), vd=vd)
                assert t.dtype == dtype and tuple(t.shape) == (d + 1, q.nq)
                assert query_grad.kernels(lat)["dots"] == [expect(vd, dtype)], (vd, dtype, query_grad.kernels(lat))
                families.add((expect(vd, dtype), dtype))
                want, T = G.dots64(v64, g, id_map(key))
                got = t.cpu().numpy().T
                assert not got[~G.ref.found].any(), (name, vd, dtype, "exactly 0 at absent corners")
                e = share(got, want, T)
                note(f"dots {dtype}", e / bar_k)
                assert e <= bar_k, (name, vd, dtype, e, bar_k)
                # an upstream gradient that is not 16-byte aligned takes the scalar loads: the same bar
                buf = torch.zeros(q.nq * vd + 4, dtype=dtype, device="cuda")
                off = buf[1:1 + q.nq * vd].view(q.nq, vd)
                off.copy_(cuda(g, NP[dtype]))
                e = share(query_grad.slice_at_dots(lat, values, q, off, vd=vd).cpu().numpy().T, want, T)
                note(f"dots {dtype}", e / bar_k)
                assert e <= bar_k, (name, vd, dtype, "unaligned", e, bar_k)
                if name == "far":
                    assert not got.any()
                if name == "train":
                    rows = np.random.default_rng(7 + d + order).permutation(n)[:q.nq]          # queries(key, "train")
                    assert np.array_equal(x[rows], Q)
                    own = v64[evid[:, inv[rows]].T]                                             # [nq, d+1, vd]
                    own_t = np.einsum("qc,qrc->qr", g.astype(np.float64), own) / L.denom
                    own_T = np.einsum("qc,qrc->qr", np.abs(g.astype(np.float64)), np.abs(own)) / L.denom
                    assert share(got, own_t, own_T) <= bar_k, (vd, dtype, "the corner order of the build")
    assert len(families) == 6
    print(f"{IDS[CASES.index(key)]}: worst share of the bars so far {WORST}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_dots_gather_nothing_at_absent_corners_and_skip_the_padding(dtype):
    """NaN planted at every vertex that no found corner references and in the stride padding of every row: the dots stay
    finite and bit-equal to those on the clean values, in every family."""
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    ref = reference(key, "jit")
    assert not ref.found.all() and ref.found.any()
    used = np.zeros(lat.m, bool)
    used[id_map(key)[ref.vid[ref.found]]] = True
    assert (~used).any()
    q = lat.locate(cuda(queries(key, "jit")))
    padded = 0
    for vd in VDS:
        values, _ = blurred(lat, x.shape[0], vd, dtype, 9)
        g = torch.randn(q.nq, vd, dtype=dtype, device="cuda", generator=torch.Generator("cuda").manual_seed(vd))
        clean = query_grad.slice_at_dots(lat, values, q, g, vd=vd)
        values[torch.from_numpy(np.nonzero(~used)[0]).cuda()] = float("nan")
        if values.shape[1] > vd:
            values[:, vd:] = float("nan")
            padded += 1
        got = query_grad.slice_at_dots(lat, values, q, g, vd=vd)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean), vd
        gx = query_grad.locate_pullback(lat, q, got)
        assert bool(torch.isfinite(gx).all())
    assert padded >= 2                                   # vd = 3 and 101 leave padding in both precisions


# ---- 2: the pull-back through the embedding ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SLICE_CASES, ids=[IDS[CASES.index(k)] for k in SLICE_CASES])
def test_pullback_of_a_given_t(key):
    """A random t, the same numbers on both sides (fp32 converts exactly): what differs is the device's rounding alone."""
    kind, d, order, lop, _ = key
    lat = gpu_lattice(key)
    for name in ("train", "jit", "fresh", "grid"):
        G = grad_ref(key, name)
        q = lat.locate(cuda(queries(key, name)))
        for dtype in (F32, F64):
            t = np.random.default_rng(23 + d).standard_normal((d + 1, q.nq)).astype(NP[dtype])
            gx = query_grad.locate_pullback(lat, q, cuda(t, NP[dtype]))
            assert gx.dtype == dtype and tuple(gx.shape) == (q.nq, d)
            t64 = t.T.astype(np.float64)
            e = share(gx.cpu().numpy(), G.pull(t64), G.terms(np.abs(t64)))
            bar_k = (d + 6) * EPS[dtype]
            note(f"pullback {dtype}", e / bar_k)
            assert e <= bar_k, (name, dtype, e, bar_k)
    assert query_grad.kernels(lat)["pullback"] == ["locate_pullback_kernel"]
    assert lat.query_kernels()["locate"] == ["locate_kernel"]


def test_rejected_queries_get_zero_rows():
    """NaN, Inf and 1e30 coordinates: a zero row whatever t holds; far queries: a zero row from their own (zero) dots."""
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    good = queries(key, "jit")[:8]
    bad = good.copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, :] = np.nan, np.inf, -np.inf, 1e30, -1e30
    q = lat.locate(cuda(bad))
    G = QueryGrad64(Query64(x, good, taps, lattice=L), taps)
    for dtype in (F32, F64):
        t = torch.randn(lat.d + 1, 8, dtype=dtype, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        gx = query_grad.locate_pullback(lat, q, t)
        assert not gx[:5].any() and bool(torch.isfinite(gx).all())
        t64 = t.cpu().numpy().T.astype(np.float64)
        assert share(gx.cpu().numpy()[5:], G.pull(t64)[5:], G.terms(np.abs(t64))[5:]) <= (lat.d + 6) * EPS[dtype]
        values, _ = blurred(lat, x.shape[0], 3, dtype, 3)
        g = torch.ones(8, 3, dtype=dtype, device="cuda")
        assert not query_grad.slice_at_backward(lat, values, q, g, vd=3)[:5].any()
        far = lat.locate(cuda(queries(key, "far")))
        assert not query_grad.slice_at_backward(lat, values, far, torch.ones(far.nq, 3, dtype=dtype, device="cuda"), vd=3).any()


# ---- 3: end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SLICE_CASES, ids=[IDS[CASES.index(k)] for k in SLICE_CASES])
def test_slice_at_backward_end_to_end(key):
    """slice_at_backward against grad64 (the geometric Jacobian, which knows no rank) on the device's own values."""
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    n = x.shape[0]
    for vd in VDS:
        for dtype in (F32, F64):
            values, v64 = blurred(lat, n, vd, dtype, 31 + vd)
            for name in ("train", "jit", "fresh", "grid", "far"):
                G = grad_ref(key, name)
                q = lat.locate(cuda(queries(key, name)))
                g = np.random.default_rng(41 + vd).standard_normal((q.nq, vd)).astype(NP[dtype])
                got = query_grad.slice_at_backward(lat, values, q, cuda(g, NP[dtype]), vd=vd)
                assert got.dtype == dtype and tuple(got.shape) == (q.nq, d)
                t64, T = G.dots64(v64, g, id_map(key))
                bar = end_to_end_bar(G, t64, T, d, vd, EPS[dtype]) + reference_error(G, t64, T, d, vd)
                e = share(got.cpu().numpy(), G.grad64(v64, g, id_map(key)), bar)
                note(f"slice_at_backward {dtype}", e)
                assert e <= 1.0, (name, vd, dtype, e)
                # ... and against the closed form of the same float64 dots under the composed bar alone: no solve in it
                e = share(got.cpu().numpy(), G.pull(t64), end_to_end_bar(G, t64, T, d, vd, EPS[dtype]))
                note(f"slice_at_backward, closed form {dtype}", e)
                assert e <= 1.0, (name, vd, dtype, "closed form", e)
                if name == "far":
                    assert not got.any()
    print(f"{IDS[CASES.index(key)]}: worst share of the bars so far {WORST}")


# ---- 4: linearity on the device ---------------------------------------------------------------------------------------
LINE_CASES = [("gauss1", 1, 3, True, None), ("gauss1", 2, 2, True, None), ("gauss1", 3, 3, False, None), ("gauss1", 8, 2, False, None),
              ("gauss1", 18, 3, False, 300)]


@pytest.mark.parametrize("key", LINE_CASES, ids=[IDS[CASES.index(k)] for k in LINE_CASES])
def test_central_differences_of_slice_at(key):
    """(slice_at(x + h e_j) - slice_at(x - h e_j)) / 2h in double values against slice_at_backward on the pairs that keep
    their corner keys: a wrong rank index or scale factor cannot pass.  h = 2^-7; at least half of the pairs are kept (a
    condition on the inputs, from the reference alone)."""
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    n, nq, vd, h = x.shape[0], 32, 3, 2.0 ** -7
    Q = queries(key, "jit")[:nq]
    base, plus, minus, kept = shifted(x, Q, taps, h, L)
    assert kept.mean() >= 0.5, kept.mean()
    G = QueryGrad64(base, taps)
    values, v64 = blurred(lat, n, vd, F64, 51)
    q = lat.locate(cuda(Q))
    back = np.zeros((nq, vd, d))
    for c in range(vd):
        g = np.zeros((nq, vd))
        g[:, c] = 1.0
        back[:, c, :] = query_grad.slice_at_backward(lat, values, q, cuda(g, np.float64), vd=vd).cpu().numpy()
    rows = G.corner_rows(v64, id_map(key))
    S = np.abs(rows).sum(1) / L.denom                                                   # [nq, vd]
    c_w = max(max(weight_error(rp, G.E, Qp), weight_error(rm, G.E, Qm)) for (Qp, rp), (Qm, rm) in zip(plus, minus))
    cap = max(max(weight_error_cap(G.s, Qp), weight_error_cap(G.s, Qm)) for (Qp, _), (Qm, _) in zip(plus, minus))
    assert c_w <= cap, (c_w, cap)
    own = np.stack([end_to_end_bar(G, np.abs(rows[:, :, c]) / L.denom, np.abs(rows[:, :, c]) / L.denom, d, vd, U2)
                    for c in range(vd)], 1)                                             # [nq, vd, d]: the backward's own bar
    worst = 0.0
    for j in range(d):
        (Qp, _), (Qm, _) = plus[j], minus[j]
        step = Qp[:, j].astype(np.float64) - Qm[:, j].astype(np.float64)
        out_p = lat.slice_at(values, lat.locate(cuda(Qp)), vd=vd).cpu().numpy()
        out_m = lat.slice_at(values, lat.locate(cuda(Qm)), vd=vd).cpu().numpy()
        cd = (out_p - out_m) / step[:, None]
        bar = (c_w * U24 + 64 * U2) * S / (step[:, None] / 2) + own[:, :, j]
        k = kept[:, j]
        worst = max(worst, share(back[k][:, :, j], cd[k], bar[k]))
    note("linearity", worst)
    print(f"{IDS[CASES.index(key)]}: kept {kept.mean():.3f}, c = {c_w:.2f}, worst share of the bar {worst:.3f}")
    assert worst <= 1.0, worst


# ---- 5: reproducibility and refusals -----------------------------------------------------------------------------------
def test_reproducible_capturable_and_row_order_free():
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    xq = cuda(queries(key, "jit"))
    lib = nv.lib()
    for dtype, vd in ((F32, 16), (F64, 3), (F32, 1), (F64, 260), (F32, 101), (F32, 260)):
        values, _ = blurred(lat, x.shape[0], vd, dtype, 1)
        q = lat.locate(xq)
        g = torch.randn(q.nq, vd, dtype=dtype, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
        t = query_grad.slice_at_dots(lat, values, q, g, vd=vd)
        gx = query_grad.locate_pullback(lat, q, t)
        assert torch.equal(query_grad.slice_at_dots(lat, values, q, g, vd=vd), t), "two calls are bit-equal"
        assert torch.equal(query_grad.slice_at_backward(lat, values, q, g, vd=vd), gx), "two calls are bit-equal"
        lat.set_lattice_row_order(True)
        try:
            assert torch.equal(query_grad.slice_at_backward(lat, values, lat.locate(xq), g, vd=vd), gx), "plx_set_row_order changes nothing"
        finally:
            lat.set_lattice_row_order(False)
        d1, nq = lat.d + 1, q.nq
        t2 = torch.full((d1, nq), -5.0, dtype=dtype, device="cuda")
        gx2 = torch.full((nq, lat.d), -7.0, dtype=dtype, device="cuda")
        dots, pull = ((lib.plx_slice_at_dots, lib.plx_locate_pullback) if dtype == F32 else
                      (lib.plx_slice_at_dots_f64, lib.plx_locate_pullback_f64))
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                sp = ctypes.c_void_p(s.cuda_stream)
                nv.check(dots(lat._h, _ptr(values), vd, _ptr(q.vid), _ptr(g), nq, _ptr(t2), sp), "plx_slice_at_dots")
                nv.check(pull(lat._h, _ptr(q.x), _ptr(t2), nq, _ptr(gx2), sp), "plx_locate_pullback")
            graph.replay()
            s.synchronize()
            assert torch.equal(t2, t) and torch.equal(gx2, gx), "graph replay"
        torch.cuda.synchronize()
        del graph


def test_between_other_entry_points_on_one_object():
    """A plx_lattice keeps tables their first user builds, scratch the builders share and value planes both precisions use
    (what tests/interleave.py drives the methods of the Lattice class body through).  The gradient's two launches the same
    way: on ONE object, after each of the entry points that share those, across a warm rebuild and a cold one, every result
    torch.equal to that of a fresh lattice which makes only that call; and a gradient call moves no bit of the entry point
    that follows it."""
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    n = x.shape[0]
    rng = np.random.default_rng(71)
    xq = cuda(queries(key, "jit"))
    src = {F32: cuda(rng.standard_normal((n, 5))), F64: cuda(rng.standard_normal((n, 5)), np.float64)}
    g = {F32: cuda(rng.standard_normal((xq.shape[0], 5))), F64: cuda(rng.standard_normal((xq.shape[0], 5)), np.float64)}

    def grad(lat, scale):
        q = lat.locate(xq * scale)
        out = []
        for dtype in (F32, F64):
            values, vd = lat.blurred(src[dtype])
            out += [query_grad.slice_at_dots(lat, values, q, g[dtype], vd=vd), query_grad.slice_at_backward(lat, values, q, g[dtype], vd=vd)]
        return out

    others = {
        "apply": lambda lat: lat.apply(src[F32]),
        "apply64": lambda lat: lat.apply(src[F64]),
        "apply_vd1": lambda lat: lat.apply(src[F32][:, :1].contiguous()),
        "rows": lambda lat: lat.apply_rows(src[F32][:n // 2].contiguous(), 0, n // 3, n // 2),
        "rows64": lambda lat: lat.apply_rows(src[F64][:n // 2].contiguous(), 0, n // 3, n // 2),
        "diag": lambda lat: lat.diag(dtype=F32),
        "diag64": lambda lat: lat.diag(dtype=F64),
        "query": lambda lat: lat.apply_at(src[F32], lat.locate(xq)),
    }

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    obj = plx.Lattice()
    first = None
    for scale, reuse in ((1.0, False), (1.05, True), (1.0, False)):
        pos = cuda(x * np.float32(scale))
        obj.build(pos, taps, reuse_order=reuse)
        twin = plx.Lattice().build(cuda(x), taps)
        if reuse:
            twin.build(pos, taps, reuse_order=True)
        want = grad(twin, scale)
        twin.close()
        assert same(grad(obj, scale), want), (scale, "the first call after a build")
        for name, other in others.items():
            other(obj)
            assert same(grad(obj, scale), want), (scale, "after", name)
            twin = plx.Lattice().build(cuda(x), taps)
            if reuse:
                twin.build(pos, taps, reuse_order=True)
            assert torch.equal(other(obj), other(twin)), (scale, name, "after a gradient call")
            twin.close()
        if first is None:
            first = want
    assert same(first, want), "the cold build on the same points again gives the first build's bits"
    obj.close()


def test_a_rebuild_makes_old_queries_stale():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = plx.Lattice().build(cuda(x), taps)
    old = lat.locate(cuda(queries(key, "jit")))
    lat.build(cuda((x / np.float32(0.6)).astype(np.float32)), taps)
    values, vd = lat.blurred(torch.ones(x.shape[0], 3, dtype=F64, device="cuda"))
    g = torch.ones(old.nq, 3, dtype=F64, device="cuda")
    for call in (lambda: query_grad.slice_at_backward(lat, values, old, g, vd=vd), lambda: query_grad.slice_at_dots(lat, values, old, g, vd=vd),
                 lambda: query_grad.locate_pullback(lat, old, torch.ones(lat.d + 1, old.nq, dtype=F64, device="cuda"))):
        with pytest.raises(RuntimeError, match="rebuilt"):
            call()
    lat.close()


def test_refusals_leave_the_outputs_untouched():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    lib = nv.lib()
    d, d1, nq, vd = lat.d, lat.d + 1, 16, 4
    xq = cuda(queries(key, "jit")[:nq])
    q = lat.locate(xq)
    unbuilt = plx.Lattice()
    oneshot = plx.Lattice()
    oneshot.filter_once(torch.ones(x.shape[0], 1, device="cuda"), cuda(x), taps)
    sharded = plx.Lattice().build(cuda(x), taps, shard=(0, 2))

    def off(t, nbytes):
        return ctypes.c_void_p(t.data_ptr() + nbytes)

    for dtype, dots, dname, pull, pname in ((F32, lib.plx_slice_at_dots, b"plx_slice_at_dots", lib.plx_locate_pullback,
                                             b"plx_locate_pullback"),
                                            (F64, lib.plx_slice_at_dots_f64, b"plx_slice_at_dots_f64",
                                             lib.plx_locate_pullback_f64, b"plx_locate_pullback_f64")):
        esz = 4 if dtype == F32 else 8
        val, _ = lat.blurred(torch.ones(x.shape[0], vd, dtype=dtype, device="cuda"))
        g = torch.ones(nq, vd, dtype=dtype, device="cuda")
        t = torch.full((d1 * nq + 4,), -5.0, dtype=dtype, device="cuda")
        gx = torch.full((nq * d + 4,), -7.0, dtype=dtype, device="cuda")
        qv = _ptr(q.vid)
        calls = [
            ((None, _ptr(val), vd, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, None, vd, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, None, _ptr(g), nq, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, qv, None, nq, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, qv, _ptr(g), nq, None), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, qv, _ptr(g), 0, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, qv, _ptr(g), -2, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), 0, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), -1, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_INVALID),
            ((lat._h, off(val, esz), vd, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_INVALID),              # vertex rows not 16-byte aligned
            ((lat._h, _ptr(val), vd, qv, off(g, 2), nq, _ptr(t)), PLX_ERR_INVALID),                # misaligned gradient
            ((lat._h, _ptr(val), vd, qv, _ptr(g), nq, off(t, 2)), PLX_ERR_INVALID),                # misaligned output
            ((lat._h, _ptr(val), vd, qv, _ptr(g), nq, _ptr(val)), PLX_ERR_INVALID),                # the output aliases the values
            ((lat._h, _ptr(val), vd, qv, _ptr(g), nq, _ptr(g)), PLX_ERR_INVALID),                  # ... the gradient
            ((unbuilt._h, _ptr(val), vd, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_STATE),
            ((oneshot._h, _ptr(val), vd, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_STATE),
            ((sharded._h, _ptr(val), vd, qv, _ptr(g), nq, _ptr(t)), PLX_ERR_STATE),
        ]
        clean_val, clean_g = val.clone(), g.clone()
        for args, code in calls:
            assert dots(*args, None) == code, (dname, args, lib.plx_last_error())
            assert dname in lib.plx_last_error()
        big = 2 ** 31 // lat.m + 8                                                              # the column limit of plx_slice_at
        assert dots(lat._h, _ptr(val), big, qv, _ptr(g), nq, _ptr(t), None) not in (0,)
        tin = torch.ones(d1, nq, dtype=dtype, device="cuda")
        calls = [
            ((None, _ptr(xq), _ptr(tin), nq, _ptr(gx)), PLX_ERR_INVALID),
            ((lat._h, None, _ptr(tin), nq, _ptr(gx)), PLX_ERR_INVALID),
            ((lat._h, _ptr(xq), None, nq, _ptr(gx)), PLX_ERR_INVALID),
            ((lat._h, _ptr(xq), _ptr(tin), nq, None), PLX_ERR_INVALID),
            ((lat._h, _ptr(xq), _ptr(tin), 0, _ptr(gx)), PLX_ERR_INVALID),
            ((lat._h, _ptr(xq), _ptr(tin), -1, _ptr(gx)), PLX_ERR_INVALID),
            ((lat._h, off(xq, 2), _ptr(tin), nq - 1, _ptr(gx)), PLX_ERR_INVALID),                  # misaligned
            ((lat._h, _ptr(xq), off(tin, 2), nq - 1, _ptr(gx)), PLX_ERR_INVALID),
            ((lat._h, _ptr(xq), _ptr(tin), nq, off(gx, 2)), PLX_ERR_INVALID),
            ((lat._h, _ptr(xq), _ptr(tin), nq, _ptr(tin)), PLX_ERR_INVALID),                       # the output aliases t
            ((unbuilt._h, _ptr(xq), _ptr(tin), nq, _ptr(gx)), PLX_ERR_STATE),
            ((oneshot._h, _ptr(xq), _ptr(tin), nq, _ptr(gx)), PLX_ERR_STATE),
            ((sharded._h, _ptr(xq), _ptr(tin), nq, _ptr(gx)), PLX_ERR_STATE),
        ]
        for args, code in calls:
            assert pull(*args, None) == code, (pname, args, lib.plx_last_error())
            assert pname in lib.plx_last_error()
        try:                                                 # reference_growth builds are refused as plx_locate refuses them
            nv.check(lib.plx_tune(b"reference_growth", 1), "plx_tune")
            grown = plx.Lattice().build(cuda(x), taps)
            if grown.reference_growth_info()["replayed"]:
                assert dots(grown._h, _ptr(val), vd, qv, _ptr(g), nq, _ptr(t), None) == PLX_ERR_STATE
                assert pull(grown._h, _ptr(xq), _ptr(tin), nq, _ptr(gx), None) == PLX_ERR_STATE
            grown.close()
        finally:
            nv.check(lib.plx_tune(b"reference_growth", 0), "plx_tune")
        torch.cuda.synchronize()
        assert bool((t == -5.0).all()) and bool((gx == -7.0).all())
        assert torch.equal(val, clean_val) and torch.equal(g, clean_g) and bool((tin == 1.0).all())
    for hnd in (unbuilt, oneshot, sharded):
        hnd.close()


# ---- 6: the autograd function ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lattice_slice_at_function(dtype):
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    vd = 5
    values, _ = blurred(lat, x.shape[0], vd, dtype, 61)
    xq = cuda(queries(key, "jit"), NP[dtype]).requires_grad_(True)
    out, mass = lattice_kernel.LatticeSliceAt.apply(xq, values, lat, vd)
    q = lat.locate(xq.detach())
    assert torch.equal(out, lat.slice_at(values, q, vd=vd)) and torch.equal(mass, q.mass), "the forward is slice_at"
    assert out.requires_grad and not mass.requires_grad
    g = torch.randn(q.nq, vd, dtype=dtype, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    (out * g).sum().backward()
    want = query_grad.slice_at_backward(lat, values, q, g, vd=vd)
    assert xq.grad.dtype == dtype and torch.equal(xq.grad, want.to(dtype))
    with pytest.raises(RuntimeError, match="adjoint splat at query points is not built"):
        lattice_kernel.LatticeSliceAt.apply(xq, values.clone().requires_grad_(True), lat, vd)
    # the positions and the values are saved for the backward: an in-place change in between is an autograd error
    xq3 = xq.detach().clone().requires_grad_(True)
    x_in = xq3 * 1.0
    out3, _ = lattice_kernel.LatticeSliceAt.apply(x_in, values, lat, vd)
    with torch.no_grad():
        x_in.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (out3 * g).sum().backward()
    # once differentiable
    xq2 = xq.detach().clone().requires_grad_(True)
    out2, _ = lattice_kernel.LatticeSliceAt.apply(xq2, values, lat, vd)
    (g1,) = torch.autograd.grad((out2 * g).sum(), xq2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


# ---- 7: PredictionCache.predict_query_grad ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_predict_query_grad(dtype):
    """n = 701, d = 3, rank-100 preconditioner, 20 Lanczos steps: d mean / d x* and d var / d x* of predict_query_grad
    against the same formulas in float64 numpy on tests/query_grad64, with the cache's own alpha, Q, chol (L), A = [alpha, Q]:

        KAQ = s K_q(x*, X) A,    DK[q, c, j] = d KAQ[q, c] / d x*_j = s sum_r J[q, r, j] V[vid_r, c] / (denom l_j),
        mean = mu + KAQ[:, 0]:                 d mean_q / d x*_j = DK[q, 0, j]
        proj = L^-1 KAQ[:, 1:]^T, var = prior - sum_k proj_k^2 (prior constant in x*):
                                               d var_q / d x*_j  = -2 sum_k proj[k, q] dproj[k, q, j],  dproj = L^-1 DK[q, 1:, j]

    with V = B_d ... B_0 S_X^T A the blurred columns in float64, J the geometric Jacobian and l the lengthscale (x* is
    divided by it before the lattice sees it).

    The bars are those of contract 6 of tests/test_query_gpu.py::test_prediction_cache, propagated.  There an entry of KAQ
    is off by beta = (b + 2 u) s terms64, b the entry bar of the product (k 2^-52 in double, ENTRY in fp32) on the size of the
    terms |S_Q| |B| ... |S_X^T| |A| / denom.  The same product error sits in the device's vertex values, bounded per vertex
    by b VT, VT = |B| ... |S_X^T| |A|; the gradient contracts the vertex values with J / l where the product contracts them
    with S_Q, so
        |d DK|   <= (b + 2 u) TK + arith =: bDK,    TK[q, c, j] = s sum_r |J[q, r, j]| VT[vid_r, c] / (denom l_j),
    arith being the end-to-end bar of the two launches (module docstring) for the upstream gradient that reaches them, plus
    3 u |DK| for the scalings by s and 1 / l:
        |d grad mean| <= bDK[:, 0, :]
        |d dproj|     <= |L^-1| bDK + t u |L^-1| |L| |dproj| =: ddp          (the solve's own backward error, Higham 8.5)
        |d grad var|  <= 2 (|proj|^T ddp + dp^T |dproj| + dp^T ddp) + 2 (t + 3) u |proj|^T |dproj|
    with dp the bar of proj of contract 6.  The device runs the adjoint order (one solve with L^T of -2 proj, then the two
    launches with that vector as upstream gradient); it is the same bilinear form, a solve with L^T obeys the same bound with
    the transposed factors, and the arithmetic terms above are doubled to cover either order.  Rows where the variance's
    clamp at 1e-8 could be active on either side (raw variance within its bar of 1e-8) are left out; at least nine in ten
    rows remain.  predict(route="query") stays torch.equal to what _predict_query computes without a graph."""
    n, d, lanc, pre = 701, 3, 20, 100
    try:
        npdt = NP[dtype]
        xn = cloud("gauss1", n, d, seed=21)
        x = cuda(xn, npdt)
        gen = torch.Generator().manual_seed(6)
        y = (torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=gen, dtype=dtype).cuda())
        xs = cuda((xn[:150] + 0.05 * np.random.default_rng(3).standard_normal((150, d))).astype(np.float32), npdt)
        model = _model(d, dtype)
        cache = training.PredictionCache(model, x, y, cg_tol=1e-6, lanc_iter=lanc, pre_size=pre)
        mean0, var0 = cache.predict(xs, route="query")
        lat, values, vd, _ = cache._query
        # predict(route="query") is what it was: the formulas of _predict_query on the raw calls
        with torch.no_grad():
            ls_t = model.kernel.lengthscale
            q0 = lat.locate(xs.div(ls_t))
            KAQ0 = model.outputscale * lat.slice_at(values, q0, vd=vd)
            proj0 = torch.linalg.solve_triangular(cache.chol, KAQ0[:, 1:].t(), upper=False)
            prior0 = model.outputscale * model.kernel(xs, xs, diag=True)
            assert torch.equal(mean0, model.mean + KAQ0[:, 0])
            assert torch.equal(var0, (prior0 - (proj0 ** 2).sum(0)).clamp_min(1e-8))

        xg = xs.clone().requires_grad_(True)
        mean, var = cache.predict_query_grad(xg)
        assert mean.requires_grad and var.requires_grad
        assert torch.equal(mean.detach(), mean0) and torch.equal(var.detach(), var0)
        assert torch.equal(cache.last_query_mass, q0.mass)
        (gm,) = torch.autograd.grad(mean.sum(), xg, retain_graph=True)
        (gv,) = torch.autograd.grad(var.sum(), xg)
        assert gm.dtype == gv.dtype == dtype and tuple(gm.shape) == tuple(gv.shape) == (150, d)
        assert all(p.grad is None for p in model.parameters()), "only x* is differentiated"
        assert query_grad.kernels(lat) == {"dots": [expect(vd, dtype)], "pullback": ["locate_pullback_kernel"]}

        # the reference, from the cache's own state
        taps = model.kernel.dkernel_fn.get_coeffs().detach().cpu().numpy()
        ls = ls_t.detach().double().cpu().numpy().reshape(-1) * np.ones(d)
        Xs = x.div(ls_t).detach().float().cpu().numpy()
        Qs = xs.div(ls_t).detach().float().cpu().numpy()
        ref = Query64(Xs, Qs, taps)
        G = QueryGrad64(ref, taps)
        assert 0.5 <= ref.found_share
        A = torch.cat([cache.alpha, cache.Q], 1).double().cpu().numpy()
        s, mu = float(model.outputscale.detach()), float(model.mean.detach())
        Lc = cache.chol.double().cpu().numpy()
        t = Lc.shape[0]
        Lat = ref.lattice
        V = ref.blurred64(A)
        VT = abs(Lat.S.T) @ np.abs(A)
        for B in Lat.blurs:
            VT = abs(B) @ VT
        rows, rowsT = G.corner_rows(V), G.corner_rows(VT)                                    # [nq, d+1, vd]
        DK = s * np.einsum("qrc,qrj->qcj", rows, G.J_geo) / ref.denom / ls                   # [nq, vd, d]
        TK = s * np.einsum("qrc,qrj->qcj", rowsT, np.abs(G.J_geo)) / ref.denom / ls
        KAQ, T = s * ref.apply64(A), s * ref.terms64(A)
        proj = scipy.linalg.solve_triangular(Lc, KAQ[:, 1:].T, lower=True)                   # [t, nq]
        dproj = np.stack([scipy.linalg.solve_triangular(Lc, DK[:, 1:, j].T, lower=True) for j in range(d)], 2)   # [t, nq, d]
        want_gm = DK[:, 0, :]
        want_gv = -2 * np.einsum("kq,kqj->qj", proj, dproj)
        prior = (model.outputscale * model.kernel(xs, xs, diag=True)).detach().double().cpu().numpy()
        raw_var = prior - (proj ** 2).sum(0)

        u = EPS[dtype]
        b = depth(lat) * U2 if dtype == F64 else ENTRY
        Linv = np.abs(np.linalg.inv(Lc))
        beta = (b + 2 * u) * T
        dp = Linv @ beta[:, 1:].T + t * u * (Linv @ (np.abs(Lc) @ np.abs(proj)))             # contract 6
        bar_var = 2 * (np.abs(proj) * dp).sum(0) + (dp * dp).sum(0) + (t + 3) * u * (np.abs(prior) + (proj ** 2).sum(0))

        def arith(g64):
            """The end-to-end bar of the two launches for the upstream gradient g64 [nq, vd] (in x* units), doubled."""
            t64, Tt = G.dots64(V, g64)
            return 2 * end_to_end_bar(G, t64, Tt, d, vd, u) / ls

        onehot = np.zeros((150, vd))
        onehot[:, 0] = s
        bar_gm = (b + 2 * u) * TK[:, 0, :] + arith(onehot) + 6 * u * np.abs(DK[:, 0, :])
        gup = np.zeros((150, vd))
        gup[:, 1:] = -2 * s * scipy.linalg.solve_triangular(Lc.T, proj, lower=False).T      # the adjoint's upstream gradient
        bDK = (b + 2 * u) * TK + 6 * u * np.abs(DK)
        ddp = np.stack([Linv @ bDK[:, 1:, j].T + t * u * (Linv @ (np.abs(Lc) @ np.abs(dproj[:, :, j]))) for j in range(d)], 2)
        bar_gv = (2 * (np.einsum("kq,kqj->qj", np.abs(proj), ddp) + np.einsum("kq,kqj->qj", dp, np.abs(dproj))
                       + np.einsum("kq,kqj->qj", dp, ddp))
                  + 4 * (t + 3) * u * np.einsum("kq,kqj->qj", np.abs(proj), np.abs(dproj)) + arith(gup))
        free = raw_var - bar_var > 1e-8                                                      # the clamp is inactive on both sides
        assert free.mean() >= 0.9, free.mean()
        em = share(gm.double().cpu().numpy(), want_gm, bar_gm)
        ev = share(gv.double().cpu().numpy()[free], want_gv[free], bar_gv[free])
        rel = np.median(bar_gv[free] / np.maximum(np.abs(want_gv[free]), 1e-300))
        print(f"predict_query_grad {dtype}: found share {ref.found_share:.3f}; d mean worst {em:.3f} of its bar, d var worst "
              f"{ev:.3f} of its bar (bar / |d var| median {rel:.2e}); clamp-free rows {free.mean():.3f}")
        note(f"prediction d mean {dtype}", em)
        note(f"prediction d var {dtype}", ev)
        assert em <= 1.0, em
        assert ev <= 1.0, ev
    finally:
        plx.lattice_cache().clear()


def test_report():
    """The worst share of every bar over the module (run as a whole)."""
    for name in sorted(WORST):
        print(f"  {name}: {WORST[name]:.3f} of its bar")
    assert all(v <= 1.0 for v in WORST.values())
