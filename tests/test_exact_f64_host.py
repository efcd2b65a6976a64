"""The float64 exact kernel MVM on the host: the four calls are declared, bound and exported; the C ABI's argument checks
(all made before any GPU work, with host pointers); the workspace bound and the split count; the Python error paths that
need no device; the case list's coverage and its named split shapes; the longdouble references against a naive loop."""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import exact as exact_mod
from tests import exact_f64 as xf

NAMES = ("plx_exact_work_bytes_f64", "plx_exact_splits_f64", "plx_exact_mvm_f64", "plx_exact_grad_f64")


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_double * 1024)()                  # host memory: every call below returns before a launch could reach it
    p = ctypes.cast(buf, ctypes.c_void_p)
    p._keep = buf
    return p


def test_symbols_and_version(lib):
    declared = _native.declared_symbols()
    for name in NAMES:
        assert name in declared and name in _native._SIGNATURES and name in _native.OPTIONAL_SYMBOLS, name
        assert hasattr(lib, name), name
    assert _native.has_symbols(*NAMES) and exact_mod.F64_SYMBOLS == NAMES
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950"
    assert _native.ABI_VERSION == (0, 9)


def test_mvm_argument_checks(lib, p):
    W = 1 << 26
    ok = dict(x1=p, n1=64, x2=p, n2=64, d=3, prof=0, v=p, t=1, out=p, work=p, wb=W)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.plx_exact_mvm_f64(a["x1"], a["n1"], a["x2"], a["n2"], a["d"], a["prof"], a["v"], a["t"], a["out"],
                                     a["work"], a["wb"], None)

    for name in ("x1", "x2", "v", "out", "work"):
        assert call(**{name: None}) == 1 and b"NULL" in lib.plx_last_error(), name
    assert b"plx_exact_mvm_f64" in lib.plx_last_error()
    assert call(d=0) == 4 and b"d = 0" in lib.plx_last_error()
    assert call(d=33) == 4 and b"d = 33" in lib.plx_last_error()
    assert call(prof=4) == 1 and b"profile" in lib.plx_last_error()
    assert call(prof=-1) == 1
    assert call(t=0) == 1 and b"t = 0" in lib.plx_last_error()
    assert call(n1=0) == 1 and call(n2=0) == 1 and call(n1=1 << 31) == 1 and call(n2=1 << 31) == 1
    assert call(n1=-5) == 1 and call(n2=-5) == 1
    # the order of the fp32 call: sizes before d, d before the profile, the profile before t
    assert call(n1=0, d=0) == 1 and call(d=0, prof=9) == 4 and call(prof=9, t=0) == 1 and b"profile" in lib.plx_last_error()
    need = lib.plx_exact_work_bytes_f64(64, 64, 3, 1)
    assert need > 0
    assert call(wb=need - 1) == 1 and b"workspace" in lib.plx_last_error() and b"plx_exact_work_bytes_f64" in lib.plx_last_error()


def test_grad_argument_checks(lib, p):
    W = 1 << 26
    ok = dict(x1=p, n1=64, x2=p, n2=64, d=3, prof=2, g=p, v=p, t=5, out=p, work=p, wb=W)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.plx_exact_grad_f64(a["x1"], a["n1"], a["x2"], a["n2"], a["d"], a["prof"], a["g"], a["v"], a["t"],
                                      a["out"], a["work"], a["wb"], None)

    for name in ("x1", "x2", "g", "v", "out", "work"):
        assert call(**{name: None}) == 1 and b"NULL" in lib.plx_last_error(), name
    assert b"plx_exact_grad_f64" in lib.plx_last_error()
    assert call(d=0) == 4 and call(d=33) == 4
    assert call(prof=7) == 1 and b"profile" in lib.plx_last_error()
    assert call(prof=-1) == 1
    assert call(t=0) == 1 and b"t = 0" in lib.plx_last_error()
    assert call(n1=0) == 1 and call(n2=0) == 1 and call(n1=1 << 31) == 1 and call(n2=1 << 31) == 1
    assert call(n1=-5) == 1 and call(n2=-5) == 1
    assert call(wb=lib.plx_exact_work_bytes_f64(64, 64, 3, 5) - 1) == 1 and b"workspace" in lib.plx_last_error()


SIZES_N = [1, 2, 7, 8, 255, 256, 257, 777, 3001, 5000, 65536, 100_000, 262_145, 1_000_000, 2_049_280, (1 << 31) - 1]
REFUSED = [(0, 10, 3, 1), (10, 0, 3, 1), (10, 10, 0, 1), (10, 10, 33, 1), (10, 10, 3, 0), (1 << 31, 10, 3, 1),
           (10, 1 << 31, 3, 1), (-1, 10, 3, 1), (10, -1, 3, 1), (10, 10, -2, 1), (10, 10, 3, -1)]


def test_work_bytes_limits_and_monotone(lib):
    for args in REFUSED:
        assert lib.plx_exact_work_bytes_f64(*args) == -1 and lib.plx_exact_work_bytes(*args) == -1, args
    ds, ts = [1, 3, 8, 18, 32], [1, 3, 11, 64, 257, 4096]
    for n2 in [1, 511, 512, 5000, 200_000, 2_000_000]:
        for d in ds:
            for t in ts:
                w = [lib.plx_exact_work_bytes_f64(n1, n2, d, t) for n1 in SIZES_N]
                assert all(b > 0 and b % 8 == 0 for b in w) and w == sorted(w), (n2, d, t, w)
                assert all((b >= 0) == (lib.plx_exact_work_bytes(n1, n2, d, t) >= 0) for n1, b in zip(SIZES_N, w))
    for n1 in SIZES_N[::3]:
        w = [lib.plx_exact_work_bytes_f64(n1, n2, 8, 11) for n2 in SIZES_N]
        assert w == sorted(w), (n1, w)
        w = [lib.plx_exact_work_bytes_f64(n1, 5000, d, 11) for d in range(1, 33)]
        assert w == sorted(w), (n1, w)
        w = [lib.plx_exact_work_bytes_f64(n1, 5000, 8, t) for t in ts]
        assert w == sorted(w), (n1, w)
    assert max(lib.plx_exact_work_bytes_f64(n, n, 32, 4096) for n in SIZES_N) <= 16 << 20
    assert lib.plx_exact_work_bytes_f64((1 << 31) - 1, (1 << 31) - 1, 32, 1 << 30) == 16 << 20


def test_splits_limits_and_workspace(lib):
    """the split count is refused exactly where the workspace bound is, and its slabs (n1 max(d, t) doubles each) fit the
    workspace at every size pair (a call of one slice writes its output directly and uses no workspace)"""
    for args in REFUSED:
        assert lib.plx_exact_splits_f64(*args) == -1, args
    assert lib.plx_exact_splits_f64(4096, 4096, 3, 1) == 8 and lib.plx_exact_splits_f64(64, 511, 3, 1) == 1
    assert lib.plx_exact_splits_f64(1_000_000, 1_000_000, 3, 1) == 1
    sizes = [1, 7, 8, 255, 256, 257, 3001, 65536, 262_145, 524_288, 524_289, 2_049_280, (1 << 31) - 1]
    for n1 in sizes:
        for n2 in sizes:
            for d, t in ((1, 1), (3, 1), (32, 1), (3, 11), (8, 64), (18, 257), (32, 4096), (1, 5_000_000)):
                s = lib.plx_exact_splits_f64(n1, n2, d, t)
                assert 1 <= s <= xf.MAX_SPLITS and (s == 1 or s <= max(1, n2 // xf.SPLIT_J)), (n1, n2, d, t, s)
                if s > 1:
                    assert 8 * s * n1 * max(d, t) <= lib.plx_exact_work_bytes_f64(n1, n2, d, t), (n1, n2, d, t, s)
                assert s <= max(1, lib.plx_exact_splits(n1, n2, d, t)), "doubles under the same cap: never more slices than fp32"


def test_python_error_paths_without_a_device():
    x = torch.randn(10, 3, dtype=torch.float64)
    v = torch.randn(10, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU path"):
        plx.exact_matmul(x, x, v, "rbf")
    with pytest.raises(ValueError, match="no CPU path"):
        plx.RBFExact().double()(x, x) @ v
    for trio in ((x.float(), x, v), (x, x.float(), v), (x, x, v.float()), (x.float(), x.float(), v)):
        with pytest.raises(TypeError, match="one dtype"):
            plx.exact_matmul(*trio, "rbf")
    with pytest.raises(ValueError, match="no CPU path"):
        plx.exact_matmul(x.float(), x.float(), v.float(), "rbf")


def test_exact_twin_follows_the_dtype():
    k = plx.RBFLattice(order=1).double()
    k.lengthscale = 0.8
    t = plx.exact_twin(k)
    assert t.lengthscale.dtype == torch.float64 and torch.allclose(t.lengthscale, k.lengthscale, rtol=4 * 2.0 ** -52, atol=0)
    m = plx.MaternLattice(nu=1.5, ard_num_dims=3)
    assert plx.exact_twin(m).lengthscale.dtype == torch.float32
    assert plx.exact_twin(m.double()).lengthscale.dtype == torch.float64


def test_source_matches_the_restated_ladders():
    src = xf.parse_source()
    assert src["dp"] == set(xf.DPS) and src["tc"] == set(xf.TCS)
    assert src["tile"] == {"float": 128, "double": xf.TILE} and xf.TILE == 64 and src["threads"] == xf.THREADS and src["split_j"] == xf.SPLIT_J and src["max_splits"] == xf.MAX_SPLITS
    for rule, fn, top in ((src["dp_rule"], xf.ex_dp, 32), (src["tc_rule"], xf.ex_tc, 70)):
        steps, default = rule
        for z in range(1, top + 1):
            assert fn(z) == next((val for bound, val in steps if z <= bound), default), z
    assert {dp: (lo, hi) for dp, (lo, hi) in xf.D_ENDS.items()} == \
        {dp: (min(d for d in range(1, 33) if xf.ex_dp(d) == dp), max(d for d in range(1, 33) if xf.ex_dp(d) == dp)) for dp in xf.DPS}


def test_case_list_covers_every_family(lib):
    reached = {xf.family(c.kind, c.profile, c.d, c.t, lib.plx_exact_splits_f64(c.n1, c.n2, c.d, c.t))
               for c in xf.CASES + xf.CAP_CASES}
    assert xf.missing_coverage(reached) == []
    assert len(xf.FAMILIES) == 224 and len(xf.EDGE_GROUPS) == 56
    # dropping one family's cases shows in the report
    one = ("grad", "matern32", 20, 8)
    assert one in xf.missing_coverage({f for f in reached if f[:4] != one})
    assert ("mvm", "rbf", "TC", 8, "slabs") in xf.missing_coverage({f for f in reached if not (f[:2] == ("mvm", "rbf") and f[3] == 8 and f[4] == "slabs")})
    tile = xf.TILE
    for group in xf.EDGE_GROUPS:
        cases = [c for c in xf.CASES if c.group == group]
        kind, dp = cases[0].kind, xf.ex_dp(cases[0].d)
        edge = [c for c in cases if (c.n1, c.n2) != xf.SPLIT_RAGGED]
        assert {c.d for c in edge} == set(xf.D_ENDS[dp]) and {c.t for c in edge} == set(xf.T_EDGES), group
        assert {c.n1 for c in edge} == set(xf.N1_EDGES) == {1, 255, 256, 257}
        assert {c.n2 for c in edge} == {1, tile - 1, tile, tile + 1, 150} and 150 > 2 * tile
        assert {c.data for c in edge} == set(xf.DATA)
        assert all(lib.plx_exact_splits_f64(c.n1, c.n2, c.d, c.t) == 1 for c in edge)
        ragged = [c for c in cases if (c.n1, c.n2) == xf.SPLIT_RAGGED]
        assert {xf.ex_tc(c.t) for c in ragged} == (set(xf.TCS) if kind == "mvm" else {xf.ex_tc(ragged[0].t)}) and len(ragged) >= 1
        assert all(c.t % xf.ex_tc(c.t) != 0 or c.t == 1 for c in ragged)
    for tc in xf.TCS:                                   # t at both ends of every TC; one, two and three column blocks
        ts = [t for t in xf.T_EDGES if xf.ex_tc(t) == tc]
        assert min(ts) == min(t for t in range(1, 40) if xf.ex_tc(t) == tc) and (tc == 16 or max(ts) == tc)
    assert {-(-t // 16) for t in xf.T_EDGES if t > 8} == {1, 2, 3}


def test_named_split_shapes(lib):
    tile = xf.TILE
    # (a) two slices, neither a multiple of the tile, two row blocks -- at every (d, t) the ragged cases use
    n1, n2 = xf.SPLIT_RAGGED
    for c in xf.CASES:
        if (c.n1, c.n2) == (n1, n2):
            assert lib.plx_exact_splits_f64(n1, n2, c.d, c.t) == 2, c
    chunk = -(-n2 // 2)
    assert chunk % tile != 0 and (n2 - chunk) % tile != 0 and chunk > tile and -(-n1 // xf.THREADS) == 2
    # (b) the maximum split count, the last slice empty; the gradient's slabs fill the workspace exactly
    n1, n2, d, t, s = xf.SPLIT_EMPTY
    assert s == xf.MAX_SPLITS == lib.plx_exact_splits_f64(n1, n2, d, t)
    chunk = -(-n2 // s)
    assert (s - 1) * chunk >= n2 > (s - 2) * chunk
    assert 8 * s * n1 * max(d, t) == lib.plx_exact_work_bytes_f64(n1, n2, d, t)
    # (c) a split count set by the 16 MiB cap, below what n2 / kEx64SplitJ would allow
    n1, n2, d, t, s = xf.SPLIT_CAP
    assert lib.plx_exact_splits_f64(n1, n2, d, t) == s
    allowed = min(xf.MAX_SPLITS, n2 // xf.SPLIT_J, -(-2048 // -(-n1 // xf.THREADS)))
    w = max(d, t)
    assert s < allowed and 8 * s * n1 * w <= xf.WORK_CAP_BYTES < 8 * (s + 1) * n1 * w
    assert lib.plx_exact_work_bytes_f64(n1, n2, d, t) == xf.WORK_CAP_BYTES
    chunk = -(-n2 // s)
    assert lib.plx_exact_splits_f64(n1, chunk, d, t) == 1 and lib.plx_exact_splits_f64(n1, n2 - (s - 1) * chunk, d, t) == 1
    assert s != lib.plx_exact_splits(n1, n2, d, t), "the double workspace holds fewer slabs than the fp32 one"
    assert [c.group for c in xf.CAP_CASES] == ["split-cap-mvm", "split-cap-grad"] and xf.CAP_ROWS == (0, 1, 255, 256)


def test_data_is_off_the_fp32_grid():
    for c in xf.CASES[::37] + [c for c in xf.CASES if c.data == "coincident"][:3]:
        data = xf.make_data(c)
        for k in ("x1", "x2", "v", "g"):
            assert data[k].dtype == np.float64 and xf.off_fp32_grid(data[k]), (c, k)
        base = xf.x64.make_data(c)
        assert all(np.abs(data[k] - base[k]).max() <= 2.0 ** -29 * max(1e-30, np.abs(base[k]).max()) for k in data)
        assert all(np.array_equal(data[k] == 0, base[k] == 0) for k in data)
        if c.data == "coincident" and c.n1 > 1:
            assert np.array_equal(data["x1"][0], data["x2"][0]) and np.array_equal(data["x1"][(c.n1 + 1) // 2 - 1], data["x2"][0])
    assert not xf.off_fp32_grid(np.array([0.5, 1.25]))


def _naive(x1, x2, g, v, profile):
    """the header's formulas as plain double loops"""
    n1, n2, d, t = x1.shape[0], x2.shape[0], x1.shape[1], v.shape[1]
    out, Tm, grad, Tg = np.zeros((n1, t)), np.zeros((n1, t)), np.zeros((n1, d)), np.zeros((n1, d))
    for i in range(n1):
        for j in range(n2):
            diff = x1[i] - x2[j]
            d2 = float(diff @ diff)
            r = np.sqrt(d2)
            if profile == "rbf":
                k, dk2, a = np.exp(-d2), -2 * np.exp(-d2), d2
            elif profile == "matern12":
                k, dk2, a = np.exp(-r), (-np.exp(-r) / r if r > 0 else 0.0), r
            elif profile == "matern32":
                s = np.sqrt(3.0) * r
                k, dk2, a = (1 + s) * np.exp(-s), -3 * np.exp(-s), s
            else:
                s = np.sqrt(5.0) * r
                k, dk2, a = (1 + s + 5.0 / 3.0 * d2) * np.exp(-s), -5.0 / 3.0 * (1 + s) * np.exp(-s), s
            out[i] += k * v[j]
            Tm[i] += k * np.abs(v[j]) * (1 + a)
            grad[i] += dk2 * diff * float(g[i] @ v[j])
            Tg[i] += abs(dk2) * np.abs(diff) * float(np.abs(g[i]) @ np.abs(v[j])) * (1 + a)
    return out, Tm, grad, Tg


@pytest.mark.parametrize("profile", xf.PROFILES)
@pytest.mark.parametrize("data", xf.DATA)
def test_longdouble_references_against_a_naive_loop(profile, data):
    c = xf.Case("tiny", "mvm", profile, 3, 5, 9, 13, data)
    z = xf.make_data(c)
    out, Tm, grad, Tg = _naive(z["x1"], z["x2"], z["g"], z["v"], profile)
    got, T = xf.mvm_ld(z["x1"], z["x2"], z["v"], profile)
    assert got.dtype == np.longdouble and T.dtype == np.longdouble
    assert xf.entry_ratio(out, got, T) <= 40 * xf.U and np.allclose(np.float64(T), Tm, rtol=1e-12, atol=0)
    got, T = xf.grad_ld(z["x1"], z["x2"], z["g"], z["v"], profile)
    assert xf.entry_ratio(grad, got, T) <= 40 * xf.U and np.allclose(np.float64(T), Tg, rtol=1e-12, atol=0)
    if data == "coincident":
        assert bool((np.float64(Tg) >= 0).all()) and np.isfinite(np.float64(got)).all()


def test_entry_ratio_and_bar():
    T = np.array([1.0, 0.0, 2.0])
    assert xf.entry_ratio([1.0, 0.0, 2.0], [1.0, 0.0, 2.0], T) == 0.0
    assert xf.entry_ratio([1.0, 1e-300, 2.0], [1.0, 0.0, 2.0], T) == float("inf")
    assert xf.entry_ratio([1.0, 1e-300, 2.0], [1.0, 0.0, 2.0], T, floor=1e-299) == 0.0
    assert xf.entry_ratio([np.nan, 0.0, 2.0], [1.0, 0.0, 2.0], T) == float("inf")
    assert xf.entry_ratio([1.0, 0.0, 2.5], [1.0, 0.0, 2.0], T) == 0.25
    # the difference is taken in longdouble: a reference half an ulp off a double is seen
    want = np.longdouble(1) + np.longdouble(2.0 ** -54)
    assert 0 < xf.entry_ratio([1.0], [want], [1.0]) <= 2.0 ** -54
    assert xf.bar("mvm", 3, 1, 64, 1) == (64 + 4 + 12 + 1 + 1) * xf.U
    assert xf.bar("mvm", 32, 33, 1500, 2) == (64 + 32 + 12 + 12 + 2) * xf.U
    assert xf.bar("grad", 9, 33, 150, 1) == (64 + 12 + 12 + 16 + 2 + 3 * 3 + 1) * xf.U
    assert max(xf.bar(c.kind, c.d, c.t, c.n2, 1) for c in xf.CASES if c.n2 <= 150) <= 150 * xf.U
