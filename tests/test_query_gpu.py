"""Queries at points that are not the build's, on the GPU: plx_locate (locate_kernel, plx_build.hip), plx_slice_at /
plx_slice_at_f64 (plx_query_kernels.h), Lattice.locate / slice_at / blurred / apply_at and PredictionCache's query route.

Yardstick: tests/query64.Query64 -- K_q(Q, X) = S_Q B_d ... B_0 S_X^T / (1 + 2^-d) in float64 from the CPU oracle's
structure (tests/test_query64.py pins it against tests/lattice64 on the CPU).

Bars, derived, not measured:
  locate      exact: -1 exactly where the reference has it, the device's key of every found id equal to the reference key,
              weights and mass torch.equal (the embedding is the build's code, compiled without contraction);
  bits        slice_at at queries that are rows of X is torch.equal to those rows of slice_rows (fp32) / slice (float64):
              the same terms in the same order from the same helpers;
  slice_at    per entry (d + 3) eps |S_Q| |values| / (1 + 2^-d), eps = 2^-24 or 2^-52: two roundings per term (the product
              and the fused multiply-add, or the product and the addition), d additions, one spare (the rounded
              reciprocal in fp32, the division in double);
  apply_at    float64 against Query64.apply64 under k 2^-52 terms64 with the k of tests/test_f64_gpu.py (depth()); fp32
              against the native float64 result under ENTRY / REL of tests/test_forward_fp64.py: the arithmetic is that of
              the product those bars were set on;
  prediction  see test_prediction_cache.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg
import torch

import simplex_gp_amd as plx
from oracle import oracle
from simplex_gp_amd import _native as nv
from simplex_gp_amd import solvers, training
from tests.lattice64 import Lattice64, cloud, entry_ratio, rel_l2
from tests.query64 import Query64, device_ids
from tests.sym64 import taps_of
from tests.test_f64_gpu import depth
from tests.test_forward_fp64 import ENTRY, REL

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EPS = {F32: 2.0 ** -24, F64: 2.0 ** -52}
U2 = 2.0 ** -52
PLX_ERR_INVALID, PLX_ERR_STATE = 1, 5
DS, ORDERS = (1, 2, 3, 8), (0, 1, 2, 3)
CLOUDS = ("gauss1", "simplex", "isolated", "dup", "grid")
N_OF = {"gauss1": 701, "simplex": 130, "isolated": 100, "dup": 300, "grid": 301}
NQ = 200
SETS = ("train", "jit", "fresh", "far", "grid")
VDS = (1, 3, 16, 101, 260)


def _cases():
    """Every (d, order, tap kind) with d in DS; the clouds rotate as in tests/test_diag_gpu.py.  Then d = 18, order 3 at
    n = 300: an odd count of key words."""
    cases = [(CLOUDS[(a + b + 2 * lop) % 5], d, order, bool(lop), None)
             for a, d in enumerate(DS) for b, order in enumerate(ORDERS) for lop in (0, 1)]
    return cases + [("gauss1", 18, 3, False, 300)]


CASES = _cases()
IDS = [f"{c}-d{d}-o{o}-{'lop' if l else 'sym'}" for c, d, o, l, _ in CASES]
_OPS, _LATS, _REFS, _IDMAPS = {}, {}, {}, {}
SHARES = {}                                   # case -> found share of its jit queries (the reference's)
WORST = {}                                    # contract -> worst error / bar


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


def cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def operator(key):
    """(positions, taps, Lattice64) of a case, computed once."""
    if key not in _OPS:
        kind, d, order, lop, n = key
        taps = taps_of(order, lop)
        x = cloud(kind, n or N_OF[kind], d, seed=3 + d + order, coeffs=taps)
        _OPS[key] = (x, taps, Lattice64(x, taps))
    return _OPS[key]


def gpu_lattice(key):
    if key not in _LATS:
        x, taps, _ = operator(key)
        _LATS[key] = plx.Lattice().build(cuda(x), taps)
    return _LATS[key]


def queries(key, name):
    """The query set `name` of a case: float32 [nq, d]."""
    kind, d, order, lop, _ = key
    x, taps, _ = operator(key)
    nq = min(NQ, x.shape[0])
    rng = np.random.default_rng(7 + d + order)
    if name == "train":
        return x[rng.permutation(x.shape[0])[:nq]].copy()
    if name == "jit":
        return (x[:nq] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32)
    if name == "fresh":
        return cloud(kind, nq, d, seed=1003 + d + order, coeffs=taps)
    if name == "far":
        # the cloud moved along the first axis past its own extent plus 12 blur steps (a step moves a key coordinate by d,
        # cloud("isolated") spaces its points like that): no corner in common, the keys well inside int16
        sf = oracle.scale_factors(d, taps)
        far = x[:nq].copy()
        far[:, 0] += np.float32(x[:, 0].max() - x[:, 0].min() + 12.0 * d / float(sf[0]))
        return far
    if name == "grid":
        return cloud("grid", nq, d, seed=2003 + d + order)             # half-integer ties
    raise ValueError(name)


def reference(key, name):
    if (key, name) not in _REFS:
        x, taps, L = operator(key)
        _REFS[key, name] = Query64(x, queries(key, name), taps, lattice=L)
    return _REFS[key, name]


def id_map(key):
    """The device's id of every vertex in the oracle's numbering of X (the device numbers along a Morton curve where it
    renumbers; the keys are the same set)."""
    if key not in _IDMAPS:
        ref = reference(key, "train")
        _IDMAPS[key] = device_ids(ref.xkeys, gpu_lattice(key).export(nv.ARRAY_KEYS))
    return _IDMAPS[key]


def slice_matrix(key, name):
    """S_Q in the device's numbering."""
    return reference(key, name).slice_matrix(id_map(key))


# ---- contract 1: locate against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_locate_against_the_reference(key):
    """Fails without the feature."""
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    assert lat.m == L.m and lat.d == d and lat.order == order
    dev_keys = lat.export(nv.ARRAY_KEYS)
    for name in SETS:
        ref = reference(key, name)
        q = lat.locate(cuda(queries(key, name)))
        assert q.nq == ref.nq and q.build_id == lat.build_id and tuple(q.vid.shape) == tuple(q.weight.shape) == (d + 1, ref.nq)
        assert q.vid.dtype == torch.int32 and q.weight.dtype == F32 and q.mass.dtype == F32
        vid = q.vid.cpu().numpy().T.astype(np.int64)
        assert vid.min() >= -1 and vid.max() < lat.m
        assert np.array_equal(vid >= 0, ref.found), (name, "-1 exactly where the reference has it")
        assert np.array_equal(dev_keys[vid[ref.found]], ref.qkeys[ref.found]), (name, "keys of the found ids")
        assert torch.equal(q.weight.cpu(), torch.from_numpy(np.ascontiguousarray(ref.weight.T))), (name, "weights")
        assert torch.equal(q.mass.cpu(), torch.from_numpy(ref.mass32)), (name, "mass")
        assert lat.locate(cuda(queries(key, name)), want_mass=False).mass is None
        if name == "train":
            assert ref.found.all()
        if name == "far":
            assert not ref.found.any() and not q.mass.any()
        if name == "jit":
            SHARES[key] = ref.found_share
            if d <= 8:                      # a condition on the inputs: the reference alone
                assert 0.5 <= ref.found_share <= 1.0, ref.found_share
    assert lat.query_kernels()["locate"] == ["locate_kernel"]


def test_the_jit_cases_hold_their_conditions():
    """At least one jit case per d >= 2 has an absent corner (the reference alone; every case at d <= 8 finds at least half
    of its corners: asserted per case above, recomputed here so that the test stands alone)."""
    for d in (2, 3, 8, 18):
        shares = [reference(key, "jit").found_share for key in CASES if key[1] == d]
        assert min(shares) < 1.0, (d, shares)
        if d <= 8:
            assert min(shares) >= 0.5, (d, shares)
    print({IDS[i]: round(reference(key, "jit").found_share, 3) for i, key in enumerate(CASES)})


def test_bad_queries_find_nothing_and_leave_the_lattice_usable():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = plx.Lattice().build(cuda(x), taps)
    good = queries(key, "jit")[:8]
    bad = good.copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, :] = np.nan, np.inf, -np.inf, 1e30, -1e30
    q = lat.locate(cuda(bad))
    vid, mass = q.vid.cpu().numpy().T, q.mass.cpu().numpy()
    assert (vid[:5] == -1).all() and (mass[:5] == 0).all()
    ref = Query64(x, good, taps, lattice=L)
    assert np.array_equal(vid[5:] >= 0, ref.found[5:]) and np.array_equal(mass[5:], ref.mass32[5:])
    values, vd = lat.blurred(cuda(np.random.default_rng(0).standard_normal((x.shape[0], 3))))
    out = lat.slice_at(values, q, vd=vd)
    assert not out[:5].any() and torch.isfinite(out).all()
    # the build's error flag was not touched: the next build on this object succeeds
    lat.build(cuda(x), taps)
    assert lat.m == L.m
    lat.close()


# ---- contract 2: bits against the existing slices -----------------------------------------------------------------------
def expect(vd, dtype):
    """The family: by the row width alone (chunks of 16 bytes)."""
    nch = (vd + 3) // 4 if dtype == F32 else (vd + 1) // 2
    return "slice_at_v1_kernel" if vd == 1 else "slice_at_chunk_kernel" if nch <= 64 else "slice_at_wide_kernel"


BIT_CASES = [("gauss1", 1, 3, True, None), ("gauss1", 3, 1, True, None), ("dup", 8, 0, False, None),
             ("gauss1", 8, 2, False, None), ("gauss1", 18, 3, False, 300)]


@pytest.mark.parametrize("key", BIT_CASES, ids=[IDS[CASES.index(k)] for k in BIT_CASES])
def test_bits_against_the_existing_slices(key):
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    n = x.shape[0]
    rng = np.random.default_rng(11)
    rows = rng.permutation(n)[:min(NQ, n)]
    q = lat.locate(cuda(x[rows]))
    assert bool((q.vid >= 0).all())
    rows_t = torch.from_numpy(rows).cuda()
    families = set()
    for vd in VDS:
        src = rng.standard_normal((n, vd))
        for dtype in (F32, F64):
            values, _ = lat.blurred(cuda(src, np.float32 if dtype == F32 else np.float64))
            full = lat.slice_rows(values, 0, n, vd=vd) if dtype == F32 else lat.slice(values, vd=vd)
            got = lat.slice_at(values, q, vd=vd)
            assert got.dtype == dtype and tuple(got.shape) == (len(rows), vd)
            assert torch.equal(got, full[rows_t]), (vd, dtype)
            assert lat.query_kernels()["slice_at"] == [expect(vd, dtype)], (vd, dtype, lat.query_kernels())
            families.add((expect(vd, dtype), dtype))
            # an output that is not 16-byte aligned takes the unaligned store: the same values
            buf = torch.full((len(rows) * vd + 4,), -7.0, dtype=dtype, device="cuda")
            off = buf[1:1 + len(rows) * vd].view(len(rows), vd)
            assert torch.equal(lat.slice_at(values, q, out=off, vd=vd), got) and float(buf[0]) == -7.0
            assert bool((buf[1 + len(rows) * vd:] == -7.0).all())
    assert len(families) == 6


# ---- contract 3: slice_at alone -----------------------------------------------------------------------------------------
SLICE_CASES = [k for k in CASES if (k[1], k[2]) in ((1, 1), (2, 2), (3, 3), (8, 1), (8, 2), (18, 3), (3, 0), (2, 1))]


@pytest.mark.parametrize("key", SLICE_CASES, ids=[IDS[CASES.index(k)] for k in SLICE_CASES])
def test_slice_at_every_entry(key):
    """Every entry of slice_at on the device's own blurred values, both precisions, every family, against
    S_Q values / (1 + 2^-d) in float64 under (d + 3) eps |S_Q| |values| / (1 + 2^-d)."""
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    n = x.shape[0]
    rng = np.random.default_rng(5)
    for vd in (1, 3, 16, 260):
        src = rng.standard_normal((n, vd))
        for dtype in (F32, F64):
            values, _ = lat.blurred(cuda(src, np.float32 if dtype == F32 else np.float64))
            v64 = values[:lat.m, :vd].cpu().numpy().astype(np.float64)
            for name in ("jit", "fresh", "far", "grid"):
                ref = reference(key, name)
                S = slice_matrix(key, name)
                q = lat.locate(cuda(queries(key, name)))
                got = lat.slice_at(values, q, vd=vd).cpu().numpy()
                want, T = (S @ v64) / L.denom, (abs(S) @ np.abs(v64)) / L.denom
                e = entry_ratio(got, want, T)                 # inf unless got is exactly 0 wherever no term reaches
                bar = (d + 3) * EPS[dtype]
                note(f"slice_at {dtype}", e / bar)
                assert e <= bar, (name, vd, dtype, e, bar)
                if name == "far":
                    assert not got.any()
    print(f"{IDS[CASES.index(key)]}: worst share of the bar so far {WORST}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_an_absent_corner_is_skipped_not_multiplied(dtype):
    """NaN planted at every vertex that no found corner of the query set references: the output stays finite and equal to
    the output on the clean values, in every family -- although the set has absent corners (ids -1)."""
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    ref = reference(key, "jit")
    assert not ref.found.all() and ref.found.any()
    used = np.zeros(lat.m, bool)
    used[id_map(key)[ref.vid[ref.found]]] = True
    assert (~used).any(), "the query set leaves some vertex unreferenced"
    q = lat.locate(cuda(queries(key, "jit")))
    rng = np.random.default_rng(9)
    for vd in (1, 3, 16, 260):
        values, _ = lat.blurred(cuda(rng.standard_normal((x.shape[0], vd)), np.float32 if dtype == F32 else np.float64))
        clean = lat.slice_at(values, q, vd=vd)
        values[torch.from_numpy(np.nonzero(~used)[0]).cuda()] = float("nan")
        got = lat.slice_at(values, q, vd=vd)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean), vd


# ---- contract 4: end to end -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_apply_at_end_to_end(key):
    kind, d, order, lop, _ = key
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    n = x.shape[0]
    vd = (1, 3, 16)[(d + order) % 3]
    v = np.random.default_rng(13 + d).standard_normal((n, vd))
    k = depth(lat)
    for name in ("train", "jit", "fresh", "far"):
        ref = reference(key, name)
        q = lat.locate(cuda(queries(key, name)))
        want, T = ref.apply64(v), ref.terms64(v)
        got64 = lat.apply_at(cuda(v, np.float64), q).cpu().numpy()
        e = entry_ratio(got64, want, T)
        note("apply_at f64", e / (k * U2))
        assert e <= k * U2, (name, "float64 entry", e, k * U2)
        got32 = lat.apply_at(cuda(v, np.float32), q).cpu().numpy()
        v32 = v.astype(np.float32).astype(np.float64)
        native = lat.apply_at(cuda(v32, np.float64), q).cpu().numpy()          # the native double product of the SAME fp32 input
        e32 = entry_ratio(got32, native, ref.terms64(v32))
        note("apply_at f32 entry", e32 / ENTRY)
        assert e32 <= ENTRY, (name, "fp32 entry", e32)
        if np.linalg.norm(native) > 0:
            r32 = rel_l2(got32, native)
            note("apply_at f32 rel", r32 / REL)
            assert r32 <= REL, (name, "fp32 rel-L2", r32)
        else:
            assert not got32.any() and not got64.any()
    print(f"{IDS[CASES.index(key)]}: k = {k}; worst share of the bars so far {WORST}")


# ---- contract 5: reproducibility and state ------------------------------------------------------------------------------
def test_reproducible_capturable_and_row_order_free():
    key = ("gauss1", 3, 3, False, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    xq = cuda(queries(key, "jit"))
    for dtype, vd in ((F32, 16), (F64, 3), (F32, 1), (F64, 260)):
        values, _ = lat.blurred(cuda(np.random.default_rng(1).standard_normal((x.shape[0], vd)),
                                     np.float32 if dtype == F32 else np.float64))
        q = lat.locate(xq)
        eager = lat.slice_at(values, q, vd=vd)
        q2 = lat.locate(xq)
        assert torch.equal(q.vid, q2.vid) and torch.equal(q.weight, q2.weight) and torch.equal(q.mass, q2.mass)
        assert torch.equal(lat.slice_at(values, q2, vd=vd), eager), "two calls are bit-equal"
        lat.set_lattice_row_order(True)
        try:
            q3 = lat.locate(xq)
            assert torch.equal(q.vid, q3.vid) and torch.equal(q.weight, q3.weight)
            assert torch.equal(lat.slice_at(values, q3, vd=vd), eager), "plx_set_row_order changes nothing"
        finally:
            lat.set_lattice_row_order(False)
        # a captured graph replays the two launches
        d1, nq = lat.d + 1, xq.shape[0]
        vid = torch.full((d1, nq), -5, dtype=torch.int32, device="cuda")
        w = torch.full((d1, nq), -5.0, device="cuda")
        mass = torch.full((nq,), -5.0, device="cuda")
        out = torch.full((nq, vd), -7.0, dtype=dtype, device="cuda")
        fn = nv.lib().plx_slice_at if dtype == F32 else nv.lib().plx_slice_at_f64
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                sp = ctypes.c_void_p(s.cuda_stream)
                nv.check(nv.lib().plx_locate(lat._h, _ptr(xq), nq, _ptr(vid), _ptr(w), _ptr(mass), sp), "plx_locate")
                nv.check(fn(lat._h, _ptr(values), vd, _ptr(vid), _ptr(w), nq, _ptr(out), sp), "plx_slice_at")
            graph.replay()
            s.synchronize()
            assert torch.equal(vid, q.vid) and torch.equal(w, q.weight) and torch.equal(mass, q.mass), "graph replay"
            assert torch.equal(out, eager), "graph replay"
        torch.cuda.synchronize()
        del graph


def test_a_rebuild_makes_old_queries_stale():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = plx.Lattice().build(cuda(x), taps)
    Q = queries(key, "jit")
    old = lat.locate(cuda(Q))
    src = np.random.default_rng(2).standard_normal((x.shape[0], 3))
    x2 = (x / np.float32(0.6)).astype(np.float32)
    Q2 = (Q / np.float32(0.6)).astype(np.float32)
    lat.build(cuda(x2), taps)                                           # another lengthscale, the same object
    values, vd = lat.blurred(cuda(src, np.float64))
    with pytest.raises(RuntimeError, match="rebuilt"):
        lat.slice_at(values, old, vd=vd)
    fresh = lat.locate(cuda(Q2))
    ref = Query64(x2, Q2, taps)
    got = lat.slice_at(values, fresh, vd=vd).cpu().numpy()
    e = entry_ratio(got, ref.apply64(src), ref.terms64(src))
    assert e <= depth(lat) * U2, e
    assert np.array_equal((fresh.vid.cpu().numpy().T >= 0), ref.found)
    lat.close()


def test_refusals_leave_the_outputs_untouched():
    key = ("gauss1", 3, 1, True, None)
    x, taps, L = operator(key)
    lat = gpu_lattice(key)
    lib = nv.lib()
    d1, nq, vd = lat.d + 1, 16, 4
    xq = cuda(queries(key, "jit")[:nq])
    q = lat.locate(xq)
    vid = torch.full((d1, nq), -5, dtype=torch.int32, device="cuda")
    w = torch.full((d1, nq), -5.0, device="cuda")
    mass = torch.full((nq,), -5.0, device="cuda")
    out32 = torch.full((nq * vd + 4,), -7.0, device="cuda")
    out64 = torch.full((nq * vd + 4,), -7.0, dtype=F64, device="cuda")
    val32, _ = lat.blurred(torch.ones(x.shape[0], vd, device="cuda"))
    val64, _ = lat.blurred(torch.ones(x.shape[0], vd, dtype=F64, device="cuda"))
    unbuilt = plx.Lattice()
    oneshot = plx.Lattice()
    oneshot.filter_once(torch.ones(x.shape[0], 1, device="cuda"), cuda(x), taps)
    sharded = plx.Lattice().build(cuda(x), taps, shard=(0, 2))

    def off(t, nbytes):
        return ctypes.c_void_p(t.data_ptr() + nbytes)

    locate_calls = [
        ((None, _ptr(xq), nq, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_INVALID),
        ((lat._h, None, nq, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_INVALID),
        ((lat._h, _ptr(xq), nq, None, _ptr(w), _ptr(mass)), PLX_ERR_INVALID),
        ((lat._h, _ptr(xq), nq, _ptr(vid), None, _ptr(mass)), PLX_ERR_INVALID),
        ((lat._h, _ptr(xq), 0, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_INVALID),
        ((lat._h, _ptr(xq), -3, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_INVALID),
        ((lat._h, off(xq, 2), nq - 1, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_INVALID),          # misaligned
        ((lat._h, _ptr(xq), nq, off(vid, 2), _ptr(w), _ptr(mass)), PLX_ERR_INVALID),
        ((lat._h, _ptr(xq), nq, _ptr(vid), _ptr(vid), _ptr(mass)), PLX_ERR_INVALID),              # outputs alias
        ((lat._h, _ptr(w), nq, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_INVALID),                 # an output aliases the input
        ((lat._h, _ptr(xq), nq, _ptr(vid), _ptr(w), _ptr(w)), PLX_ERR_INVALID),
        ((unbuilt._h, _ptr(xq), nq, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_STATE),
        ((oneshot._h, _ptr(xq), nq, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_STATE),
        ((sharded._h, _ptr(xq), nq, _ptr(vid), _ptr(w), _ptr(mass)), PLX_ERR_STATE),
    ]
    for args, code in locate_calls:
        assert lib.plx_locate(*args, None) == code, (args, lib.plx_last_error())
        assert b"plx_locate" in lib.plx_last_error()
    torch.cuda.synchronize()
    assert bool((vid == -5).all()) and bool((w == -5.0).all()) and bool((mass == -5.0).all())

    for fn, name, val, out, esz in ((lib.plx_slice_at, b"plx_slice_at", val32, out32, 4),
                                    (lib.plx_slice_at_f64, b"plx_slice_at_f64", val64, out64, 8)):
        qv, qw = _ptr(q.vid), _ptr(q.weight)
        calls = [
            ((None, _ptr(val), vd, qv, qw, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, None, vd, qv, qw, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, None, qw, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, qv, None, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, qv, qw, nq, None), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), vd, qv, qw, 0, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), 0, qv, qw, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, _ptr(val), -1, qv, qw, nq, _ptr(out)), PLX_ERR_INVALID),
            ((lat._h, off(val, esz), vd, qv, qw, nq, _ptr(out)), PLX_ERR_INVALID),                 # vertex rows not 16-byte aligned
            ((lat._h, _ptr(val), vd, qv, qw, nq, off(out, 2)), PLX_ERR_INVALID),                   # misaligned output
            ((lat._h, _ptr(val), vd, qv, qw, nq, _ptr(val)), PLX_ERR_INVALID),                     # the output aliases the values
            ((unbuilt._h, _ptr(val), vd, qv, qw, nq, _ptr(out)), PLX_ERR_STATE),
            ((oneshot._h, _ptr(val), vd, qv, qw, nq, _ptr(out)), PLX_ERR_STATE),
            ((sharded._h, _ptr(val), vd, qv, qw, nq, _ptr(out)), PLX_ERR_STATE),
        ]
        clean = val.clone()
        for args, code in calls:
            assert fn(*args, None) == code, (name, args, lib.plx_last_error())
            assert name in lib.plx_last_error()
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and torch.equal(val, clean)
    # the column limit of plx_slice_rows / plx_slice_f64: m * stride below 2^31
    big = 2 ** 31 // lat.m + 8
    assert lib.plx_slice_at(lat._h, _ptr(val32), big, _ptr(q.vid), _ptr(q.weight), nq, _ptr(out32), None) not in (0,)
    assert lib.plx_slice_rows(lat._h, _ptr(val32), big, 0, nq, _ptr(out32), None) not in (0,)
    torch.cuda.synchronize()
    assert bool((out32 == -7.0).all())
    # reference_growth builds are refused like the diagonal refuses them
    try:
        nv.check(lib.plx_tune(b"reference_growth", 1), "plx_tune")
        grown = plx.Lattice().build(cuda(x), taps)
        if grown.reference_growth_info()["replayed"]:
            assert lib.plx_locate(grown._h, _ptr(xq), nq, _ptr(vid), _ptr(w), _ptr(mass), None) == PLX_ERR_STATE
            assert lib.plx_slice_at(grown._h, _ptr(val32), vd, _ptr(q.vid), _ptr(q.weight), nq, _ptr(out32), None) == PLX_ERR_STATE
        grown.close()
    finally:
        nv.check(lib.plx_tune(b"reference_growth", 0), "plx_tune")
    torch.cuda.synchronize()
    assert bool((vid == -5).all()) and bool((out32 == -7.0).all())
    for h in (unbuilt, oneshot, sharded):
        h.close()


# ---- contract 6: PredictionCache ------------------------------------------------------------------------------------------
def _model(d, dtype, noise=0.1):
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d))
    model = (model.double() if dtype == F64 else model).cuda()
    with torch.no_grad():
        model.raw_noise.fill_(float(np.log(np.expm1(noise - model.min_noise))))
    return model


def _parent_predict(cache, x_star):
    """PredictionCache.predict as it stood before the query route: the formulas of the parent, on the cache's own state."""
    model = cache.model
    K_star = model.kernel(x_star, cache.x)
    s = model.outputscale
    KAQ = s * K_star.matmul(torch.cat([cache.alpha, cache.Q], 1).contiguous())
    mean = model.mean + KAQ[:, 0]
    proj = torch.linalg.solve_triangular(cache.chol, KAQ[:, 1:].t(), upper=False)
    prior = s * model.kernel(x_star, x_star, diag=True)
    return mean, (prior - (proj ** 2).sum(0)).clamp_min(1e-8)


class Counter:
    """Wraps a call of the loaded library and counts."""

    def __init__(self, monkeypatch, name):
        self.calls = 0
        real = getattr(nv.lib(), name)

        def counted(*a):
            self.calls += 1
            return real(*a)

        monkeypatch.setattr(nv.lib(), name, counted)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_prediction_cache(monkeypatch, dtype):
    """n = 701, d = 3, rank-100 preconditioner, 20 Lanczos steps.

    route="query" against the same formulas in float64 numpy on tests/query64, with the cache's own alpha, Q, chol (L):
        KAQ = s K_q(x*, X) [alpha, Q],  mean = mu + KAQ[:, 0],  proj = L^-1 KAQ[:, 1:]^T,  var = max(prior - sum proj^2, 1e-8).
    With u the unit roundoff of the model's dtype and b the entry bar of contract 4 (k 2^-52 in double, ENTRY in fp32),
    an entry of KAQ is off by at most beta = (b + 2 u) s terms64 (the product's bar, the scaling by s and the conversion of
    s), so
        |d mean|  <= beta_0 + 2 u (|mu| + |KAQ_0|)                                       (the addition of mu)
        |d proj|  <= |L^-1| beta + t u |L^-1| |L| |proj|  =: dp                           (the right-hand side's error through the
                     solve, and the solve's own backward error: a triangular solve of t rows, Higham 8.5, gamma_t ~ t u)
        |d var|   <= 2 |proj|^T dp + dp^T dp + (t + 3) u (|prior| + sum proj^2)          (the squares, their sum, the difference,
                     the prior's own scaling)
    where the reference clamps at 1e-8 the bar is taken before the clamp (the clamp is 1-Lipschitz).  Both are derived;
    the measured worst shares are printed.
    route="stacked" and the default are torch.equal to the parent's formulas on the same cache; last_query_mass is
    locate's mass; a second batch builds nothing and splats nothing."""
    n, d, lanc, pre = 701, 3, 20, 100
    try:
        npdt = np.float64 if dtype == F64 else np.float32
        xn = cloud("gauss1", n, d, seed=21)
        x = cuda(xn, npdt)
        g = torch.Generator().manual_seed(6)
        y = (torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=g, dtype=dtype).cuda())
        xs = cuda((xn[:150] + 0.05 * np.random.default_rng(3).standard_normal((150, d))).astype(np.float32), npdt)
        xs2 = cuda(cloud("gauss1", 90, d, seed=22), npdt)
        model = _model(d, dtype)
        cache = training.PredictionCache(model, x, y, cg_tol=1e-6, lanc_iter=lanc, pre_size=pre)
        assert cache.Q is not None and cache.Q.dtype == dtype and training.PredictionCache.query_route is False

        # the default and "stacked": the parent's formulas, bit for bit
        pm, pv = _parent_predict(cache, xs)
        for route in (None, "stacked"):
            m_, v_ = cache.predict(xs) if route is None else cache.predict(xs, route=route)
            assert torch.equal(m_, pm) and torch.equal(v_, pv), route
            assert cache.last_query_mass is None and "_query" not in cache.__dict__

        mean, var = cache.predict(xs, route="query")
        lat, values, vd, bid = cache._query
        assert vd == 1 + cache.Q.shape[1] and values.dtype == dtype and bid == lat.build_id
        ls = model.kernel.lengthscale
        assert torch.equal(cache.last_query_mass, lat.locate(xs.div(ls)).mass)
        assert lat.query_kernels()["slice_at"] == [expect(vd, dtype)]

        # the reference, from the cache's own state
        taps = model.kernel.dkernel_fn.get_coeffs().detach().cpu().numpy()
        Xs = x.div(ls).detach().float().cpu().numpy()
        Qs = xs.div(ls).detach().float().cpu().numpy()
        ref = Query64(Xs, Qs, taps)
        assert 0.5 <= ref.found_share and np.array_equal(cache.last_query_mass.cpu().numpy(), ref.mass32)
        A = torch.cat([cache.alpha, cache.Q], 1).double().cpu().numpy()
        s, mu = float(model.outputscale), float(model.mean)
        Lc = cache.chol.double().cpu().numpy()
        KAQ, T = s * ref.apply64(A), s * ref.terms64(A)
        prior = (model.outputscale * model.kernel(xs, xs, diag=True)).detach().double().cpu().numpy()
        proj = scipy.linalg.solve_triangular(Lc, KAQ[:, 1:].T, lower=True)
        want_mean, raw_var = mu + KAQ[:, 0], prior - (proj ** 2).sum(0)
        u = EPS[dtype]
        b = depth(lat) * U2 if dtype == F64 else ENTRY
        beta = (b + 2 * u) * T
        bar_mean = beta[:, 0] + 2 * u * (abs(mu) + np.abs(KAQ[:, 0]))
        t = Lc.shape[0]
        Linv = np.abs(np.linalg.inv(Lc))
        dp = Linv @ beta[:, 1:].T + t * u * (Linv @ (np.abs(Lc) @ np.abs(proj)))
        bar_var = 2 * (np.abs(proj) * dp).sum(0) + (dp * dp).sum(0) + (t + 3) * u * (np.abs(prior) + (proj ** 2).sum(0))
        em = np.abs(mean.double().cpu().numpy() - want_mean) / bar_mean
        ev = np.abs(var.double().cpu().numpy() - np.maximum(raw_var, 1e-8)) / bar_var
        print(f"PredictionCache {dtype}: found share {ref.found_share:.3f}; mean worst {em.max():.3f} of its bar, variance "
              f"worst {ev.max():.3f} of its bar (bar / |var| median {np.median(bar_var / np.maximum(np.abs(raw_var), 1e-8)):.2e})")
        note(f"prediction mean {dtype}", em.max())
        note(f"prediction variance {dtype}", ev.max())
        assert em.max() <= 1.0, em.max()
        assert ev.max() <= 1.0, ev.max()

        # a second batch: no build, no splat, no blur -- the library is not asked, and what it last reported stands
        lat.splat(torch.ones(n, 1, dtype=dtype, device="cuda"))          # a marker: the single-column splat
        names = (lat.stage_kernels(), lat.f64_kernels())
        counters = [Counter(monkeypatch, name) for name in ("plx_build", "plx_splat", "plx_splat_f64", "plx_blur",
                                                            "plx_blur_f64", "plx_splat_rows", "plx_splat_rows_f64")]
        c_loc = Counter(monkeypatch, "plx_locate")
        c_at = Counter(monkeypatch, "plx_slice_at_f64" if dtype == F64 else "plx_slice_at")
        prior_counter = Counter(monkeypatch, "plx_apply_rows")
        m2, v2 = cache.predict(xs2, route="query")
        assert [c.calls for c in counters] == [0] * len(counters)
        assert (c_loc.calls, c_at.calls, prior_counter.calls) == (1, 1, 0)
        assert cache._query[3] == bid == lat.build_id and cache._query[1] is values
        assert (lat.stage_kernels(), lat.f64_kernels()) == names
        assert lat.query_kernels() == {"locate": ["locate_kernel"], "slice_at": [expect(vd, dtype)]}
        assert tuple(m2.shape) == tuple(v2.shape) == (90,) and tuple(cache.last_query_mass.shape) == (90,)
        assert bool(torch.isfinite(m2).all()) and bool(torch.isfinite(v2).all())
        # the class switch routes the default
        monkeypatch.setattr(training.PredictionCache, "query_route", True)
        m3, v3 = cache.predict(xs2)
        assert torch.equal(m3, m2) and torch.equal(v3, v2)
        m4, v4 = cache.predict(xs2, route="stacked")
        assert cache.last_query_mass is None and tuple(m4.shape) == (90,)
    finally:
        plx.lattice_cache().clear()


def test_report():
    """The worst share of every bar over the module (run as a whole)."""
    for name in sorted(WORST):
        print(f"  {name}: {WORST[name]:.3f} of its bar")
    assert all(v <= 1.0 for v in WORST.values())
