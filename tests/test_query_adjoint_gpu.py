"""The splat at query points on the GPU: plx_query_plan, plx_splat_at / plx_splat_at_f64 (plx_query_adjoint.hip over the
kernels of plx_rows.hip / plx_rows_f64.hip), query_adjoint.plan / splat_at / slice_at_adjoint / apply_at_t, and
LatticeSliceAtValues / LatticeQueryProduct.

Yardstick: tests/query_adjoint64.QueryAdjoint64 on tests/query64.Query64 (pinned on the CPU by tests/test_query_adjoint64.py,
which also asserts the conditions on the inputs used here).  c_v: the found query corners at vertex v; eps = 2^-24 / 2^-52.

Bars, derived, not measured:
  splat_at     per entry (c_v + 1) eps (|S_Q|^T |g|)[v]: a vertex sums c_v products, each rounded once or fused, in c_v - 1
               additions: c_v units, one spare.  Exactly 0 where no corner lands and in the stride padding.
  own splat    splat_at at Q = X within 2 (c_v + 1) eps T_v of Lattice.splat: the same terms in another order, each side
               within the bar above.  No reference.
  identity     <slice_at_adjoint(g), V> against <g, slice_at(V)>, both dots in longdouble on the CPU: the sum over v of
               (c_v + 3) eps (|S_Q|^T |g|)[v] |V_v| / denom (the division of g and its product with V's entry are the two
               further units) plus the sum over q of (d + 3) eps (|S_Q| |V|)[q] |g_q| / denom, slice_at's own bar.
  apply_at_t   float64 against apply_t64 under k_t 2^-52 terms_t64, k_t = max(cmax, 1) + (2r + 1)(d + 1) + 2 (d + 1) + 8:
               depth() of tests/test_f64_gpu.py with the query splat's depth for the build's; fp32 against the native
               double result of the same fp32 input under (ENTRY + cmax 2^-24) terms_t64, ENTRY the project's bar of the
               transposed fp32 chain (tests/sym32.py), the second summand the share of a splat depth that bar was not set on.
Everything else is promised exactly.  Fails without the feature."""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import lattice_kernel, query_adjoint, query_grad
from tests.lattice64 import Lattice64, cloud, entry_ratio
from tests.query64 import Query64, device_ids
from tests.query_adjoint64 import ALL_ABSENT, DEPTH_CASE, SPLAT_CASES, SPLAT_SETS, QueryAdjoint64
from tests.sym32 import ENTRY
from tests.sym64 import taps_of
from tests.test_query_gpu import CASES, EPS, IDS, SLICE_CASES, VDS, cuda, gpu_lattice, id_map, operator, queries, reference, slice_matrix

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NP = {F32: np.float32, F64: np.float64}
U2 = 2.0 ** -52
PLX_ERR_INVALID, PLX_ERR_STATE, PLX_ERR_TOO_LARGE = 1, 5, 6
WORST = {}


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def expect(vd, dtype):
    """The family: by the row width alone (chunks of 16 bytes)."""
    nch = (vd + 3) // 4 if dtype == F32 else (vd + 1) // 2
    stem = "rows_splat" if dtype == F32 else "rows64_splat"
    return stem + ("_v1_kernel" if vd == 1 else "_chunk_kernel" if nch <= 64 else "_wide_kernel")


def tables(plan, m, P):
    """(ptr [m + 1], row [P], w [P]) of a plan: the first three sections of its buffer, each rounded up to 256 bytes."""
    up = lambda b: (b + 255) & ~255
    o_row = up(4 * (m + 1))
    o_w = o_row + up(4 * P)
    buf = plan.buffer
    return (buf[:4 * (m + 1)].view(torch.int32), buf[o_row:o_row + 4 * P].view(torch.int32), buf[o_w:o_w + 4 * P].view(F32))


def same_plan(a, b, m, P):
    return all(torch.equal(u, v) for u, v in zip(tables(a, m, P), tables(b, m, P)))


def rand32(rng, shape):
    """Normal values that are fp32 numbers: the device reads the same input in both precisions."""
    return rng.standard_normal(shape).astype(np.float32)


def check_splat(lat, ref, id_of, Q, label, families, vds=VDS):
    """Contract 1 on one (lattice, query set): the plan's tables exactly, then splat_at per entry at every vd, both
    precisions, aligned and unaligned g, into an output prefilled with NaN."""
    m, d1, nq = lat.m, lat.d + 1, Q.shape[0]
    A = QueryAdjoint64(ref, id_of=id_of)
    q = lat.locate(cuda(Q))
    plan = query_adjoint.plan(lat, q)
    assert plan.nq == nq and plan.build_id == lat.build_id
    assert query_adjoint.kernels(lat)["plan"][0] == "query_plan_keys_kernel"
    assert "query_plan_fill_kernel" in query_adjoint.kernels(lat)["plan"] and "rows_ptr_kernel" in query_adjoint.kernels(lat)["plan"]
    # the tables: ptr from the reference's counts; row and w the stable sort of the device's own pairs by vertex
    ptr, row, w = (t.cpu().numpy() for t in tables(plan, m, nq * d1))
    assert np.array_equal(ptr, np.concatenate([[0], np.cumsum(A.counts)])), (label, "ptr")
    vid = q.vid.cpu().numpy().ravel().astype(np.int64)
    keys = np.where((vid >= 0) & (vid < m), vid, m)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(row, order % nq) and np.array_equal(w, q.weight.cpu().numpy().ravel()[order]), (label, "row, w")
    rng = np.random.default_rng(17)
    c1 = (A.counts + 1).astype(np.float64)[:, None]
    for vd in vds:
        g = rand32(rng, (nq, vd))
        want, T = A.splat_at64(g), A.splat_terms64(g).astype(np.float64)
        for dtype in (F32, F64):
            stride = lat.values_stride(vd, dtype)
            out = torch.full((m, stride), float("nan"), dtype=dtype, device="cuda")
            got_t = query_adjoint.splat_at(lat, cuda(g, NP[dtype]), q, plan=plan, values=out)
            assert got_t is out and bool(torch.isfinite(out).all()), (label, vd, dtype, "every row and padding column written")
            assert not bool(out[:, vd:].any()), (label, vd, dtype, "the stride padding is exact zeros")
            assert query_adjoint.kernels(lat)["splat_at"] == [expect(vd, dtype)], (vd, dtype, query_adjoint.kernels(lat))
            families.add((expect(vd, dtype), dtype))
            got = out[:, :vd].cpu().numpy()
            err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
            e = entry_ratio(err, np.zeros_like(err), T * c1)     # inf unless exactly 0 wherever no corner lands
            note(f"splat_at {dtype}", e / EPS[dtype])
            assert e <= EPS[dtype], (label, vd, dtype, e, EPS[dtype])
            if A.cmax == 0:
                assert not bool(out.any()) and not ptr.any(), (label, "nothing found: all zeros, ptr all 0")
            # a gradient that is not 16-byte aligned takes the scalar loads: the same values
            buf = torch.zeros(nq * vd + 4, dtype=dtype, device="cuda")
            off = buf[1:1 + nq * vd].view(nq, vd)
            off.copy_(cuda(g, NP[dtype]))
            assert off.data_ptr() % 16 != 0
            assert torch.equal(query_adjoint.splat_at(lat, off, q, plan=plan), out), (label, vd, dtype, "unaligned g")
    return A


# ---- contract 1: splat_at, every entry ----------------------------------------------------------------------------------
FAMILIES = set()


@pytest.mark.parametrize("key", SPLAT_CASES + [DEPTH_CASE], ids=[IDS[CASES.index(k)] for k in SPLAT_CASES + [DEPTH_CASE]])
def test_splat_at_every_entry(key):
    """Fails without the feature."""
    lat = gpu_lattice(key)
    for name in SPLAT_SETS:
        A = check_splat(lat, reference(key, name), id_map(key), queries(key, name), (key, name), FAMILIES)
        if name == "far" or (key, name) in ALL_ABSENT:
            assert A.cmax == 0
    assert len(FAMILIES) == 6, FAMILIES
    print(f"{IDS[CASES.index(key)]}: worst share of the bar so far {WORST}")


def test_one_query_and_a_point_three_times():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    Q = queries(key, "jit")
    one = Q[3:4].copy()
    thrice = np.concatenate([Q[:5], Q[2:3], Q[7:9], Q[2:3]], 0)                     # row 2 three times
    for name, Qs in (("one", one), ("thrice", thrice)):
        ref = Query64(x, Qs, taps, lattice=L)
        assert ref.found.any()
        A = check_splat(lat, ref, id_map(key), Qs, name, set())
        if name == "thrice":
            assert A.cmax >= 3


# ---- contract 2: a power-of-two vertex count ------------------------------------------------------------------------------
def test_a_power_of_two_vertex_count():
    """m = 8: the absent key m = 8 needs four sorted bits, the ids up to m - 1 three."""
    taps = taps_of(1, False)
    x = cloud("gauss1", 300, 1, seed=5, coeffs=taps)
    L = Lattice64(x, taps)
    lat = plx.Lattice().build(cuda(x), taps)
    assert lat.m == L.m and lat.m & (lat.m - 1) == 0, lat.m
    rng = np.random.default_rng(8)
    jit = (x[:200] + 0.05 * rng.standard_normal((200, 1))).astype(np.float32)
    far = x[:200].copy()
    far[:, 0] += np.float32(2.0 * (x[:, 0].max() - x[:, 0].min()) + 100.0)
    mixed = np.concatenate([jit[:100], far[:100]], 0)
    families = set()
    for name, Q in (("jit", jit), ("far", far), ("mixed", mixed)):
        ref = Query64(x, Q, taps, lattice=L)
        id_of = device_ids(ref.xkeys, lat.export(nv.ARRAY_KEYS))
        A = check_splat(lat, ref, id_of, Q, ("pow2", name), families)
        assert (A.cmax == 0) == (name == "far")
        if name == "mixed":
            assert 0.0 < ref.found_share < 1.0
    lat.close()


# ---- contract 3: against the build's own splat ----------------------------------------------------------------------------
OWN_CASES = [("gauss1", 1, 3, True, None), ("dup", 8, 0, False, None), ("gauss1", 18, 3, False, 300)]


@pytest.mark.parametrize("key", OWN_CASES, ids=[IDS[CASES.index(k)] for k in OWN_CASES])
def test_against_the_builds_own_splat(key):
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    n = x.shape[0]
    q = lat.locate(cuda(x))
    assert bool((q.vid >= 0).all())
    plan = query_adjoint.plan(lat, q)
    c = np.diff(lat.export(nv.ARRAY_ROW_PTR).astype(np.int64))                     # the build's own count
    assert np.array_equal(tables(plan, lat.m, n * (lat.d + 1))[0].cpu().numpy(), np.concatenate([[0], np.cumsum(c)]))
    rng = np.random.default_rng(19)
    for vd in (1, 3, 101):
        src = rand32(rng, (n, vd))
        T = lat.splat(cuda(np.abs(src), np.float64))[:, :vd].cpu().numpy()
        for dtype in (F32, F64):
            s = cuda(src, NP[dtype])
            got = query_adjoint.splat_at(lat, s, q, plan=plan)[:, :vd].cpu().numpy()
            own = lat.splat(s)[:, :vd].cpu().numpy()
            e = entry_ratio(got, own, T * (2.0 * (c + 1))[:, None])
            note(f"own splat {dtype}", e / EPS[dtype])
            assert e <= EPS[dtype], (vd, dtype, e)


# ---- contract 4: the adjoint identity on the device ---------------------------------------------------------------------
ID_CASES = [("gauss1", 1, 3, True, None), ("gauss1", 3, 1, True, None), ("dup", 8, 0, False, None), ("gauss1", 18, 3, False, 300)]


@pytest.mark.parametrize("key", ID_CASES, ids=[IDS[CASES.index(k)] for k in ID_CASES])
def test_the_adjoint_identity_on_the_device(key):
    """A wrong weight, a wrong row index or a dropped corner cannot pass."""
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    ref = reference(key, "jit")
    A = QueryAdjoint64(ref, id_of=id_map(key))
    S = slice_matrix(key, "jit")
    q = lat.locate(cuda(queries(key, "jit")))
    plan = query_adjoint.plan(lat, q)
    rng = np.random.default_rng(23 + d)
    LD = np.longdouble
    for vd in (1, 3, 101):
        for dtype in (F32, F64):
            stride = lat.values_stride(vd, dtype)
            V = cuda(rand32(rng, (lat.m, stride)), NP[dtype])                      # NaN-free padding
            g = cuda(rand32(rng, (ref.nq, vd)), NP[dtype])
            adj = query_adjoint.slice_at_adjoint(lat, g, q, plan=plan)
            assert tuple(adj.shape) == (lat.m, stride) and not bool(adj[:, vd:].any())
            out = lat.slice_at(V, q, vd=vd)
            Vn, gn = V[:, :vd].cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
            lhs = (adj[:, :vd].cpu().numpy().astype(LD) * Vn.astype(LD)).sum()
            rhs = (gn.astype(LD) * out.cpu().numpy().astype(LD)).sum()
            bar = EPS[dtype] / L.denom * (float((((A.counts + 3)[:, None] * (abs(S).T @ np.abs(gn))) * np.abs(Vn)).sum())
                                          + float(((d + 3) * (abs(S) @ np.abs(Vn)) * np.abs(gn)).sum()))
            err = float(abs(lhs - rhs))
            note(f"identity {dtype}", err / bar)
            assert err <= bar, (vd, dtype, err, bar)


# ---- contract 5: apply_at_t end to end ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SLICE_CASES, ids=[IDS[CASES.index(k)] for k in SLICE_CASES])
def test_apply_at_t_end_to_end(key):
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    vd = (1, 3, 16)[(d + order) % 3]
    rng = np.random.default_rng(29 + d)
    for name in ("train", "jit", "fresh", "far"):
        ref = reference(key, name)
        A = QueryAdjoint64(ref, id_of=id_map(key))
        q = lat.locate(cuda(queries(key, name)))
        k_t = max(A.cmax, 1) + (2 * order + 1) * (d + 1) + 2 * (d + 1) + 8
        g = rng.standard_normal((ref.nq, vd))
        got64 = query_adjoint.apply_at_t(lat, cuda(g, np.float64), q).cpu().numpy()
        assert got64.shape == (x.shape[0], vd)
        e = entry_ratio(got64, A.apply_t64(g), A.terms_t64(g))
        note("apply_at_t f64", e / (k_t * U2))
        assert e <= k_t * U2, (name, "float64 entry", e, k_t * U2)
        g32 = g.astype(np.float32)
        got32 = query_adjoint.apply_at_t(lat, cuda(g32), q).cpu().numpy()
        native = query_adjoint.apply_at_t(lat, cuda(g32, np.float64), q).cpu().numpy()     # the native double result of the SAME input
        bar32 = ENTRY + A.cmax * 2.0 ** -24
        e32 = entry_ratio(got32, native, A.terms_t64(g32.astype(np.float64)))
        note("apply_at_t f32", e32 / bar32)
        assert e32 <= bar32, (name, "fp32 entry", e32, bar32)
        if name == "far":
            assert not got32.any() and not got64.any()
    print(f"{IDS[CASES.index(key)]}: worst share of the bars so far {WORST}")


# ---- contract 6: reproducibility and stale plans --------------------------------------------------------------------------
def test_reproducible_capturable_and_row_order_free():
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    xq = cuda(queries(key, "jit"))
    lib = nv.lib()
    m, d1, nq = lat.m, lat.d + 1, xq.shape[0]
    for dtype, vd in ((F32, 16), (F64, 3), (F32, 1), (F64, 260), (F32, 101), (F32, 260)):
        q = lat.locate(xq)
        g = torch.randn(nq, vd, dtype=dtype, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
        plan = query_adjoint.plan(lat, q)
        eager = query_adjoint.splat_at(lat, g, q, plan=plan)
        assert torch.equal(query_adjoint.splat_at(lat, g, q, plan=plan), eager), "two calls are bit-equal"
        plan2 = query_adjoint.plan(lat, lat.locate(xq))
        assert same_plan(plan, plan2, m, nq * d1), "a second plan of the same query"
        assert torch.equal(query_adjoint.splat_at(lat, g, q, plan=plan2), eager) and torch.equal(query_adjoint.splat_at(lat, g, q), eager)
        full = query_adjoint.apply_at_t(lat, g, q, plan=plan)
        lat.set_lattice_row_order(True)
        try:
            # as slice() does: the fp32 rows come back in lattice order, the float64 rows always in the caller's
            ordered = query_adjoint.apply_at_t(lat, g, q, plan=plan)
            assert torch.equal(lat.from_lattice_order(ordered) if dtype == F32 else ordered, full), "plx_set_row_order"
            assert torch.equal(query_adjoint.splat_at(lat, g, q, plan=plan), eager), "plx_set_row_order changes no vertex row"
        finally:
            lat.set_lattice_row_order(False)
        # a captured graph replays the plan and the splat: warmed up, one chain on one stream
        nbytes = int(lib.plx_query_plan_bytes(lat._h, nq))
        assert nbytes == plan.buffer.numel()
        pbuf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.full((m, lat.values_stride(vd, dtype)), -7.0, dtype=dtype, device="cuda")
        fn = lib.plx_splat_at if dtype == F32 else lib.plx_splat_at_f64
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            sp = ctypes.c_void_p(s.cuda_stream)
            nv.check(lib.plx_query_plan(lat._h, _ptr(q.vid), _ptr(q.weight), nq, _ptr(pbuf), sp), "plx_query_plan")
            nv.check(fn(lat._h, _ptr(pbuf), _ptr(g), vd, nq, _ptr(out), sp), "plx_splat_at")
            s.synchronize()
            pbuf.zero_()
            out.fill_(-7.0)
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                nv.check(lib.plx_query_plan(lat._h, _ptr(q.vid), _ptr(q.weight), nq, _ptr(pbuf), sp), "plx_query_plan")
                nv.check(fn(lat._h, _ptr(pbuf), _ptr(g), vd, nq, _ptr(out), sp), "plx_splat_at")
            graph.replay()
            s.synchronize()
            assert same_plan(query_adjoint.QueryPlan(pbuf, nq, lat.build_id), plan, m, nq * d1), "graph replay"
            assert torch.equal(out, eager), "graph replay"
        torch.cuda.synchronize()
        del graph


def test_between_other_entry_points_on_one_object():
    """On ONE object, after each of the entry points that share tables, scratch and value planes with a plx_lattice, across a
    warm rebuild and a cold one, plan + splat_at + apply_at_t are torch.equal to those of a fresh lattice that makes only
    that call; and the entry point that follows keeps its own bits."""
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    n = x.shape[0]
    rng = np.random.default_rng(73)
    xq = cuda(queries(key, "jit"))
    nq = xq.shape[0]
    src = {F32: cuda(rng.standard_normal((n, 5))), F64: cuda(rng.standard_normal((n, 5)), np.float64)}
    g = {F32: cuda(rng.standard_normal((nq, 5))), F64: cuda(rng.standard_normal((nq, 5)), np.float64)}

    def adjoint(lat, scale):
        q = lat.locate(xq * scale)
        plan = query_adjoint.plan(lat, q)
        out = list(tables(plan, lat.m, nq * (lat.d + 1)))
        for dtype in (F32, F64):
            out += [query_adjoint.splat_at(lat, g[dtype], q, plan=plan), query_adjoint.apply_at_t(lat, g[dtype], q, plan=plan)]
        return out

    def backward(lat):
        values, vd = lat.blurred(src[F64])
        return query_grad.slice_at_backward(lat, values, lat.locate(xq), g[F64], vd=vd)

    others = {
        "apply": lambda lat: lat.apply(src[F32]),
        "apply64": lambda lat: lat.apply(src[F64]),
        "rows": lambda lat: lat.apply_rows(src[F32][:n // 2].contiguous(), 0, n // 3, n // 2),
        "rows64": lambda lat: lat.apply_rows(src[F64][:n // 2].contiguous(), 0, n // 3, n // 2),
        "diag": lambda lat: lat.diag(dtype=F32),
        "slice_at": lambda lat: lat.apply_at(src[F32], lat.locate(xq)),
        "slice_at_backward": backward,
    }

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    def fresh(pos, reuse):
        twin = plx.Lattice().build(cuda(x), taps)
        return twin.build(pos, taps, reuse_order=True) if reuse else twin

    obj = plx.Lattice()
    first = None
    for scale, reuse in ((1.0, False), (1.05, True), (1.0, False)):
        pos = cuda(x * np.float32(scale))
        obj.build(pos, taps, reuse_order=reuse)
        twin = fresh(pos, reuse)
        want = adjoint(twin, scale)
        twin.close()
        assert same(adjoint(obj, scale), want), (scale, "the first call after a build")
        for name, other in others.items():
            other(obj)
            assert same(adjoint(obj, scale), want), (scale, "after", name)
            twin = fresh(pos, reuse)
            assert torch.equal(other(obj), other(twin)), (scale, name, "after an adjoint call")
            twin.close()
        if first is None:
            first = want
    assert same(first, want), "the cold build on the same points again gives the first build's bits"
    obj.close()


def test_a_rebuild_makes_old_plans_stale():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = plx.Lattice().build(cuda(x), taps)
    Q = queries(key, "jit")
    old_q = lat.locate(cuda(Q))
    old_plan = query_adjoint.plan(lat, old_q)
    g = torch.ones(old_q.nq, 3, dtype=F64, device="cuda")
    lat.build(cuda((x / np.float32(0.6)).astype(np.float32)), taps)
    new_q = lat.locate(cuda((Q / np.float32(0.6)).astype(np.float32)))
    for call in (lambda: query_adjoint.splat_at(lat, g, new_q, plan=old_plan), lambda: query_adjoint.splat_at(lat, g, old_q),
                 lambda: query_adjoint.plan(lat, old_q), lambda: query_adjoint.apply_at_t(lat, g, new_q, plan=old_plan),
                 lambda: query_adjoint.slice_at_adjoint(lat, g, old_q, plan=old_plan),
                 lambda: query_adjoint.splat_at(lat, g[:7], lat.locate(cuda(Q[:7])), plan=query_adjoint.plan(lat, new_q))):
        with pytest.raises(RuntimeError, match="rebuilt"):
            call()
    assert bool(torch.isfinite(query_adjoint.splat_at(lat, g, new_q)).all())
    lat.close()


def test_refusals_leave_the_outputs_untouched():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    lib = nv.lib()
    d1, nq, vd = lat.d + 1, 16, 4
    q = lat.locate(cuda(queries(key, "jit")[:nq]))
    good = query_adjoint.plan(lat, q)
    nbytes = good.buffer.numel()
    assert nbytes == lib.plx_query_plan_bytes(lat._h, nq) and nbytes % 256 == 0
    unbuilt = plx.Lattice()
    oneshot = plx.Lattice()
    oneshot.filter_once(torch.ones(x.shape[0], 1, device="cuda"), cuda(x), taps)
    sharded = plx.Lattice().build(cuda(x), taps, shard=(0, 2))
    huge = (2 ** 31 - 4096) // d1 + 1
    assert lib.plx_query_plan_bytes(unbuilt._h, nq) == -1 and lib.plx_query_plan_bytes(lat._h, 0) == -1
    assert lib.plx_query_plan_bytes(lat._h, -3) == -1 and lib.plx_query_plan_bytes(lat._h, huge) == -1
    assert lib.plx_query_plan_bytes(lat._h, 10 ** 6) > 4 * 7 * 10 ** 6 * d1

    def off(t, nbytes_):
        return ctypes.c_void_p(t.data_ptr() + nbytes_)

    pbuf = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    qv, qw = _ptr(q.vid), _ptr(q.weight)
    calls = [
        ((None, qv, qw, nq, _ptr(pbuf)), PLX_ERR_INVALID),
        ((lat._h, None, qw, nq, _ptr(pbuf)), PLX_ERR_INVALID),
        ((lat._h, qv, None, nq, _ptr(pbuf)), PLX_ERR_INVALID),
        ((lat._h, qv, qw, nq, None), PLX_ERR_INVALID),
        ((lat._h, qv, qw, 0, _ptr(pbuf)), PLX_ERR_INVALID),
        ((lat._h, qv, qw, -2, _ptr(pbuf)), PLX_ERR_INVALID),
        ((lat._h, off(q.vid, 2), qw, nq - 1, _ptr(pbuf)), PLX_ERR_INVALID),                        # misaligned
        ((lat._h, qv, off(q.weight, 2), nq - 1, _ptr(pbuf)), PLX_ERR_INVALID),
        ((lat._h, qv, qw, nq, off(pbuf, 4)), PLX_ERR_INVALID),                                      # the plan off its 16 bytes
        ((lat._h, qv, qw, nq, qv), PLX_ERR_INVALID),                                                # the plan overlaps an input
        ((lat._h, qv, qw, huge, _ptr(pbuf)), PLX_ERR_TOO_LARGE),
        ((unbuilt._h, qv, qw, nq, _ptr(pbuf)), PLX_ERR_STATE),
        ((oneshot._h, qv, qw, nq, _ptr(pbuf)), PLX_ERR_STATE),
        ((sharded._h, qv, qw, nq, _ptr(pbuf)), PLX_ERR_STATE),
    ]
    clean_vid, clean_w = q.vid.clone(), q.weight.clone()
    for args, code in calls:
        assert lib.plx_query_plan(*args, None) == code, (args, lib.plx_last_error())
        assert b"plx_query_plan" in lib.plx_last_error()
    torch.cuda.synchronize()
    assert bool((pbuf == 0x5A).all()) and torch.equal(q.vid, clean_vid) and torch.equal(q.weight, clean_w)

    for dtype, fn, name in ((F32, lib.plx_splat_at, b"plx_splat_at"), (F64, lib.plx_splat_at_f64, b"plx_splat_at_f64")):
        esz = 4 if dtype == F32 else 8
        g = torch.ones(nq * vd + 4, dtype=dtype, device="cuda")
        out = torch.full((lat.m * lat.values_stride(vd, dtype) + 4,), -7.0, dtype=dtype, device="cuda")
        P = _ptr(good.buffer)
        calls = [
            ((None, P, _ptr(g), vd, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, None, _ptr(g), vd, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, P, None, vd, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, P, _ptr(g), vd, nq, None), PLX_ERR_INVALID),
            ((lat._h, P, _ptr(g), vd, 0, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, P, _ptr(g), vd, -1, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, P, _ptr(g), 0, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, P, _ptr(g), -1, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, off(good.buffer, 4), _ptr(g), vd, nq, _ptr(out)), PLX_ERR_INVALID),           # the plan off its 16 bytes
            ((lat._h, P, off(g, 2), vd, nq, _ptr(out)), PLX_ERR_INVALID),                           # misaligned gradient
            ((lat._h, P, _ptr(g), vd, nq, off(out, 2)), PLX_ERR_INVALID),                           # misaligned output
            ((lat._h, P, _ptr(g), vd, nq, off(out, esz)), PLX_ERR_INVALID),                         # vertex rows off their 16 bytes
            ((lat._h, P, _ptr(g), vd, nq, _ptr(g)), PLX_ERR_INVALID),                               # the output overlaps the gradient
            ((lat._h, P, _ptr(g), vd, nq, P), PLX_ERR_INVALID),                                     # ... the plan
            ((lat._h, P, _ptr(g), 2 ** 31 // lat.m + 8, nq, _ptr(out)), PLX_ERR_TOO_LARGE),
            ((lat._h, P, _ptr(g), 1, huge, _ptr(out)), PLX_ERR_TOO_LARGE),
            ((unbuilt._h, P, _ptr(g), vd, nq, _ptr(out)), PLX_ERR_STATE),
            ((oneshot._h, P, _ptr(g), vd, nq, _ptr(out)), PLX_ERR_STATE),
            ((sharded._h, P, _ptr(g), vd, nq, _ptr(out)), PLX_ERR_STATE),
        ]
        clean_plan = good.buffer.clone()
        for args, code in calls:
            assert fn(*args, None) == code, (name, args, lib.plx_last_error())
            assert name in lib.plx_last_error()
        try:                                                 # reference_growth builds are refused as plx_locate refuses them
            nv.check(lib.plx_tune(b"reference_growth", 1), "plx_tune")
            grown = plx.Lattice().build(cuda(x), taps)
            if grown.reference_growth_info()["replayed"]:
                assert fn(grown._h, P, _ptr(g), vd, nq, _ptr(out), None) == PLX_ERR_STATE
                assert lib.plx_query_plan(grown._h, qv, qw, nq, _ptr(pbuf), None) == PLX_ERR_STATE
            grown.close()
        finally:
            nv.check(lib.plx_tune(b"reference_growth", 0), "plx_tune")
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((g == 1.0).all()) and torch.equal(good.buffer, clean_plan)
        assert bool((pbuf == 0x5A).all())
    for hnd in (unbuilt, oneshot, sharded):
        hnd.close()


# ---- contract 7: autograd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lattice_slice_at_values_function(dtype):
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    vd = 5
    rng = np.random.default_rng(61)
    values = lat.blurred(cuda(rng.standard_normal((x.shape[0], vd)), NP[dtype]))[0].clone().requires_grad_(True)
    xq = cuda(queries(key, "jit"), NP[dtype]).requires_grad_(True)
    out, mass = lattice_kernel.LatticeSliceAtValues.apply(xq, values, lat, vd)
    q = lat.locate(xq.detach())
    assert torch.equal(out, lat.slice_at(values.detach(), q, vd=vd)) and torch.equal(mass, q.mass), "the forward is slice_at"
    assert out.requires_grad and not mass.requires_grad
    g = torch.randn(q.nq, vd, dtype=dtype, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    (out * g).sum().backward()
    assert values.grad.dtype == dtype and torch.equal(values.grad, query_adjoint.slice_at_adjoint(lat, g, q))
    assert xq.grad.dtype == dtype
    assert torch.equal(xq.grad, query_grad.slice_at_backward(lat, values.detach(), q, g, vd=vd).to(dtype))
    # values alone: x gets nothing
    xq2 = xq.detach().clone()
    v2 = values.detach().clone().requires_grad_(True)
    out2, _ = lattice_kernel.LatticeSliceAtValues.apply(xq2, v2, lat, vd)
    (g1,) = torch.autograd.grad((out2 * g).sum(), v2, create_graph=True)
    assert torch.equal(g1, values.grad)
    with pytest.raises(RuntimeError):                                              # once differentiable
        g1.sum().backward()
    with pytest.raises(RuntimeError, match="adjoint splat at query points is not built"):
        lattice_kernel.LatticeSliceAt.apply(xq, values, lat, vd)                   # LatticeSliceAt itself did not change


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lattice_query_product_function(dtype):
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    vd = 5
    rng = np.random.default_rng(67)
    src = cuda(rng.standard_normal((x.shape[0], vd)), NP[dtype]).requires_grad_(True)
    xq = cuda(queries(key, "jit"), NP[dtype]).requires_grad_(True)
    out, mass = lattice_kernel.LatticeQueryProduct.apply(lat, src, xq)
    q = lat.locate(xq.detach())
    assert torch.equal(out, lat.apply_at(src.detach(), q)) and torch.equal(mass, q.mass) and not mass.requires_grad
    g = torch.randn(q.nq, vd, dtype=dtype, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    (out * g).sum().backward()
    assert src.grad.dtype == dtype and torch.equal(src.grad, query_adjoint.apply_at_t(lat, g, q))
    values, _ = lat.blurred(src.detach())
    assert torch.equal(xq.grad, query_grad.slice_at_backward(lat, values, q, g, vd=vd).to(dtype))
    src2 = src.detach().clone().requires_grad_(True)
    out2, _ = lattice_kernel.LatticeQueryProduct.apply(lat, src2, xq.detach())
    (g1,) = torch.autograd.grad((out2 * g).sum(), src2, create_graph=True)
    assert torch.equal(g1, src.grad)
    with pytest.raises(RuntimeError):                                              # once differentiable
        g1.sum().backward()


def test_gradcheck_of_the_query_product():
    """The map is linear in src and the backward is its exact transpose: torch.autograd.gradcheck in float64, src alone."""
    d, n, nq, vd = 3, 40, 12, 2
    taps = taps_of(1, False)
    x = cloud("gauss1", n, d, seed=31, coeffs=taps)
    lat = plx.Lattice().build(cuda(x), taps)
    rng = np.random.default_rng(37)
    xq = cuda((x[:nq] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32), np.float64)
    assert bool((lat.locate(xq).mass > 0).any())
    src = cuda(rng.standard_normal((n, vd)), np.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda s: lattice_kernel.LatticeQueryProduct.apply(lat, s, xq)[0], (src,))
    lat.close()


def test_report():
    """The worst share of every bar over the module (run as a whole)."""
    for name in sorted(WORST):
        print(f"  {name}: {WORST[name]:.3f} of its bar")
    assert all(v <= 1.0 for v in WORST.values())
