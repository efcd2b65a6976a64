"""The true diagonal of the lattice operator on the GPU (simplex_gp_amd/csrc/plx_diag_kernels.h: plx_diag / plx_diag_f64,
Lattice.diag) and what is built on it (SquareLazyLattice.true_diag, the preconditioners' true_diag).

Yardsticks: tests/diag64 -- diag_dense, the diagonal of the dense float64 matrix of tests/lattice64.Lattice64, and diag_terms,
the size of the terms each K_ii sums (tests/test_diag64.py pins the path identity on the CPU).

Bars, derived, not measured:
  accuracy        per entry k eps diag_terms with k = (d+1)^2 (2r+1) + d + 4 (one rounding per term of a sequential sum, the
                  roundings of a path's product, the two weight products, the division: it holds for any summation order) and
                  eps = 2^-52 (plx_diag_f64) or 2^-24 (plx_diag);
  rows, bits      torch.equal: every output element is formed by the same sums in the same order whatever the range, the
                  row order or the launch route (eager, captured graph);
  factor          LatticePreconditioner against PivotedCholeskyPreconditioner on the same diagonal: max |dL| <= 2e-4 max |L|,
                  the tolerance tests/test_pcg_native.py holds the two classes to.
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import lattice_kernel, solvers
from simplex_gp_amd._native import PlxError
from tests import diag64
from tests.lattice64 import Lattice64, cloud
from tests.sym64 import Sym64, taps_of

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EPS = {F32: 2.0 ** -24, F64: 2.0 ** -52}
PLX_ERR_INVALID, PLX_ERR_STATE = 1, 5
DS, ORDERS = (1, 2, 3, 8), (0, 1, 2, 3, 4)
CLOUDS = ("gauss1", "simplex", "isolated", "dup", "grid")
N_OF = {"gauss1": 701, "simplex": 130, "isolated": 100, "dup": 300, "grid": 301}


def _cases():
    """Every (d, order, tap kind); the clouds rotate so that each meets every d and every order."""
    return [(CLOUDS[(a + b + 2 * lop) % 5], d, order, bool(lop))
            for a, d in enumerate(DS) for b, order in enumerate(ORDERS) for lop in (0, 1)]


CASES = _cases()
IDS = [f"{c}-d{d}-o{o}-{'lop' if l else 'sym'}" for c, d, o, l in CASES]
_OPS, _LATS = {}, {}
WORST = {F32: 0.0, F64: 0.0}


def cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def operator(kind, d, order, lop, n=None):
    """(positions, Lattice64, taps, dense diagonal, terms) of a case, computed once."""
    key = (kind, d, order, lop, n)
    if key not in _OPS:
        taps = taps_of(order, lop)
        x = cloud(kind, n or N_OF[kind], d, seed=3 + d + order, coeffs=taps)
        L = Lattice64(x, taps)
        _OPS[key] = (x, L, taps, diag64.diag_dense(L), diag64.diag_terms(L))
    return _OPS[key]


def gpu_lattice(kind, d, order, lop, n=None):
    key = (kind, d, order, lop, n)
    if key not in _LATS:
        x, _, taps, _, _ = operator(*key)
        _LATS[key] = plx.Lattice().build(cuda(x, np.float32), taps)
    return _LATS[key]


def ratio(got, want, terms):
    """max |got - want| / terms over every entry."""
    assert np.all(terms > 0), "w_a^2 c_r^(d+1) > 0 for some corner of every point"
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    return float((np.abs(got - want) / terms).max())


@pytest.mark.parametrize("kind,d,order,lop", CASES, ids=IDS)
def test_every_entry_against_float64(kind, d, order, lop):
    """Both precisions, every entry, against the diagonal of the dense float64 matrix.  Fails without the feature."""
    x, L, taps, dense, terms = operator(kind, d, order, lop)
    lat = gpu_lattice(kind, d, order, lop)
    assert lat.m == L.m and lat.order == order and lat.d == d
    k = diag64.bar_terms(d, order)
    for dtype in (F64, F32):
        got = lat.diag(dtype=dtype)
        assert got.dtype == dtype and tuple(got.shape) == (L.n,)
        e = ratio(got.cpu().numpy(), dense, terms)
        WORST[dtype] = max(WORST[dtype], e / (k * EPS[dtype]))
        print(f"{kind} n={L.n} d={d} order={order} lop={lop} {dtype}: {e / EPS[dtype]:.2f} ulp of {k} "
              f"(worst share of the bar so far {WORST[dtype]:.3f}); diagonal min {dense.min():.3f} mean {dense.mean():.3f} "
              f"max {dense.max():.3f}")
        assert e <= k * EPS[dtype], (dtype, e, k * EPS[dtype])


@pytest.mark.parametrize("kind,d,order,lop", [("gauss1", 3, 1, True), ("dup", 8, 2, True), ("grid", 2, 3, False),
                                              ("simplex", 1, 4, True), ("gauss1", 8, 0, False)])
def test_against_the_device_products(kind, d, order, lop):
    """diag of apply(I), apply_t(I) and apply_sym(I) in float64 -- the device's own neighbour table and weights -- against
    diag(float64), under the bar."""
    n = 130
    x, L, taps, dense, terms = operator(kind, d, order, lop, n)
    lat = gpu_lattice(kind, d, order, lop, n)
    eye = torch.eye(n, dtype=F64, device="cuda")
    want = lat.diag(dtype=F64).cpu().numpy()
    k = diag64.bar_terms(d, order)
    kt_terms = diag64.diag_terms(Sym64(x, taps).kt)
    for name, fn, T in (("apply", lat.apply, terms), ("apply_t", lat.apply_t, kt_terms),
                        ("apply_sym", lat.apply_sym, 0.5 * (terms + kt_terms))):
        got = fn(eye).diagonal().cpu().numpy()
        e = ratio(got, want, T)
        print(f"{kind} d={d} order={order} {name}: {e / EPS[F64]:.2f} ulp of {k}")
        assert e <= k * EPS[F64], (name, e)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_row_ranges_and_lattice_rows(dtype):
    kind, d, order, lop = "gauss1", 3, 2, True
    lat = gpu_lattice(kind, d, order, lop)
    n = lat.n
    full = lat.diag(dtype=dtype)
    for begin, count in ((0, 1), (0, 97), (211, 300), (350, 1), (n - 64, 64), (n - 1, 1), (0, n)):
        part = lat.diag(dtype=dtype, rows=(begin, count))
        assert tuple(part.shape) == (count,) and torch.equal(part, full[begin:begin + count]), (begin, count)
    in_lattice_order = lat.diag(dtype=dtype, lattice_rows=True)
    assert torch.equal(in_lattice_order, full[lat.shard_perm()])
    # the flag is the call's own: plx_set_row_order changes nothing
    lat.set_lattice_row_order(True)
    try:
        assert torch.equal(lat.diag(dtype=dtype), full)
        assert torch.equal(lat.diag(dtype=dtype, lattice_rows=True), in_lattice_order)
    finally:
        lat.set_lattice_row_order(False)


def test_stacked_prediction_rows():
    """On the stacked lattice [xout; xin] the range of xin is diag K(x*, x*): the dense diagonal of the stacked matrix there."""
    d, order = 3, 1
    taps = taps_of(order, False)
    xout, xin = cloud("gauss1", 400, d, seed=5), cloud("gauss1", 123, d, seed=6)
    stacked = np.concatenate([xout, xin])
    L = Lattice64(stacked, taps)
    dense, terms = diag64.diag_dense(L), diag64.diag_terms(L)
    lat = plx.Lattice().build(cuda(stacked, np.float32), taps)
    k = diag64.bar_terms(d, order)
    for dtype in (F64, F32):
        got = lat.diag(dtype=dtype, rows=(400, 123))
        assert ratio(got.cpu().numpy(), dense[400:], terms[400:]) <= k * EPS[dtype]
    lat.close()


def test_bits_and_state():
    kind, d, order, lop = "gauss1", 8, 1, False
    x, L, taps, dense, terms = operator(kind, d, order, lop)
    lat = plx.Lattice().build(cuda(x, np.float32), taps)
    n = lat.n
    v = cuda(np.random.default_rng(1).standard_normal((n, 2)))
    lat.apply(v.float())
    lat.apply(v)
    bytes0, names0, names64 = lat.device_bytes, lat.stage_kernels(), lat.f64_kernels()
    for dtype in (F32, F64):
        out = torch.full((n,), -7.0, dtype=dtype, device="cuda")
        eager = lat.diag(dtype=dtype, out=out).clone()
        assert torch.equal(lat.diag(dtype=dtype), eager), "two calls are bit-equal"
        # a captured graph replays the one launch: the first call of a build may be the captured one
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out.fill_(-7.0)
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                lat.diag(dtype=dtype, out=out)
            graph.replay()
            s.synchronize()
            assert torch.equal(out, eager), "graph replay"
        torch.cuda.synchronize()
        del graph
    assert lat.device_bytes == bytes0 and lat.stage_kernels() == names0 and lat.f64_kernels() == names64
    # another lengthscale on the same object: the new lattice's diagonal
    x2 = (x / np.float32(0.6)).astype(np.float32)
    L2 = Lattice64(x2, taps)
    lat.build(cuda(x2, np.float32), taps)
    k = diag64.bar_terms(d, order)
    for dtype in (F64, F32):
        got = lat.diag(dtype=dtype).cpu().numpy()
        assert ratio(got, diag64.diag_dense(L2), diag64.diag_terms(L2)) <= k * EPS[dtype]
        assert ratio(got, dense, terms) > k * EPS[dtype], "the rebuilt lattice has another diagonal"
    lat.close()


def test_refusals_leave_the_output_untouched():
    n, d = 300, 3
    taps = taps_of(1, True)
    x = cuda(cloud("gauss1", n, d, seed=1, coeffs=taps), np.float32)
    lib = nv.lib()
    lat = plx.Lattice().build(x, taps)
    SENT = -12345.0
    for fn, dtype, size in ((lib.plx_diag, F32, 4), (lib.plx_diag_f64, F64, 8)):
        buf = torch.full((n + 2,), SENT, dtype=dtype, device="cuda")
        out = buf[:n]

        def refused(code, h, begin, count, lrows, ptr, word=None):
            assert fn(h, begin, count, lrows, ptr, None) == code, (begin, count, lrows)
            if word is not None:
                assert word in lib.plx_last_error(), lib.plx_last_error()
            torch.cuda.synchronize()
            assert bool((buf == SENT).all()), "a refused call wrote"

        refused(PLX_ERR_INVALID, None, 0, n, 0, _ptr(out))
        refused(PLX_ERR_INVALID, lat._h, 0, n, 0, None)
        refused(PLX_ERR_INVALID, lat._h, 0, 0, 0, _ptr(out))
        refused(PLX_ERR_INVALID, lat._h, 0, -3, 0, _ptr(out))
        refused(PLX_ERR_INVALID, lat._h, -1, 5, 0, _ptr(out))
        refused(PLX_ERR_INVALID, lat._h, n - 4, 5, 0, _ptr(out))
        refused(PLX_ERR_INVALID, lat._h, n, 1, 0, _ptr(out))
        refused(PLX_ERR_INVALID, lat._h, 0, n - 1, 1, _ptr(out), b"lattice_rows")
        refused(PLX_ERR_INVALID, lat._h, 1, n - 1, 1, _ptr(out), b"lattice_rows")
        refused(PLX_ERR_INVALID, lat._h, 0, n, 0, ctypes.c_void_p(out.data_ptr() + size // 2), b"aligned")
        fresh = plx.Lattice()
        refused(PLX_ERR_STATE, fresh._h, 0, n, 0, _ptr(out), b"not built")
        fresh.close()
        shard = plx.Lattice().build(x, taps, shard=(0, 2))
        refused(PLX_ERR_STATE, shard._h, 0, n, 0, _ptr(out), b"sharded")
        shard.close()
        nv.check(lib.plx_tune(b"reference_growth", 1), "plx_tune")
        try:
            grown = plx.Lattice().build(x, taps)
        finally:
            nv.check(lib.plx_tune(b"reference_growth", 0), "plx_tune")
        assert grown.reference_growth_info()["replayed"]
        refused(PLX_ERR_STATE, grown._h, 0, n, 0, _ptr(out), b"reference_growth")
        with pytest.raises(PlxError) as err:
            grown.diag(dtype=dtype)
        assert err.value.code == PLX_ERR_STATE
        grown.close()
        # ... and the accepted call writes its rows and nothing else
        assert fn(lat._h, 0, n, 0, _ptr(out), None) == 0
        torch.cuda.synchronize()
        assert bool((buf[n:] == SENT).all()) and bool((out != SENT).all())
    lat.close()


def test_python_interface(monkeypatch):
    lat = gpu_lattice("gauss1", 3, 2, True)
    for bad in (torch.float16, torch.bfloat16, torch.int32, None):
        with pytest.raises(TypeError, match="float32 or torch.float64"):
            lat.diag(dtype=bad)
    with pytest.raises(ValueError):
        lat.diag(rows=(0, lat.n + 1))
    with pytest.raises(ValueError, match="whole range"):
        lat.diag(rows=(0, 5), lattice_rows=True)
    assert nv.has_symbols("plx_diag", "plx_diag_f64"), "libplx.so lacks plx_diag / plx_diag_f64"
    assert {"plx_diag", "plx_diag_f64"} <= set(nv.declared_symbols())
    monkeypatch.setattr(nv, "has_symbols", lambda *names: False)
    with pytest.raises(RuntimeError, match="does not export plx_diag_f64"):
        lat.diag(dtype=F64)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_square_operator_switch(dtype):
    n, d = 500, 3
    x = cuda(cloud("gauss1", n, d, seed=4), np.float32).to(dtype)
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).cuda().to(dtype)
    with torch.no_grad():
        model.kernel.lengthscale = 0.7
        K = model.kernel(x, x)
        assert type(K) is lattice_kernel.SquareLazyLattice and lattice_kernel.SquareLazyLattice.true_diag is False
        ones = K.diag()
        assert ones.dtype == dtype and torch.equal(ones, torch.ones(n, dtype=dtype, device="cuda"))
        lattice_kernel.SquareLazyLattice.true_diag = True
        try:
            got = K.diag()
            on_cpu = type(K)(K.x.cpu(), K.dkernel).diag()
        finally:
            lattice_kernel.SquareLazyLattice.true_diag = False
        lat = lattice_kernel.lattice_cache().get(K.x, K.dkernel.get_coeffs())
        assert got.dtype == dtype and torch.equal(got, lat.diag(dtype=dtype))
        assert 0.3 < float(got.min()) and float(got.max()) < 1.0 and float(got.mean()) < 0.85
        assert torch.equal(on_cpu, torch.ones(n, dtype=dtype)), "any other case: ones, as before"
        # ... and it is the diagonal of the product this operator computes
        p = int(torch.argmax(got))
        e = torch.zeros(n, 1, dtype=dtype, device="cuda")
        e[p] = 1.0
        assert abs(float(K.matmul(e)[p]) - float(got[p])) <= 1e-5


@pytest.mark.parametrize("d,ell", [(3, 0.5), (8, 0.9)])
def test_preconditioner_on_the_true_diagonal(d, ell):
    """LatticePreconditioner(true_diag=True): the first pivot is the argmax of the true diagonal, the factor is the one the
    torch form builds from the same diagonal, and true_diag=False is today's factor to the bit."""
    n, rank = 701, 100
    x = cuda(cloud("gauss1", n, d, seed=7), np.float32)
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).cuda()
    with torch.no_grad():
        model.kernel.lengthscale = ell
        K = model.kernel(x, x)
        ref = model.preconditioner(x, rank, K=K, factor_dtype=F32)
        lat, s, noise = ref.lat, float(model.outputscale), float(model.noise)
        off = solvers.LatticePreconditioner(lat, s, noise, rank, factor_dtype=F32, true_diag=False)
        assert torch.equal(off.L, ref.L), "true_diag=False is the factor as it was"
        dk = lat.diag()
        got = solvers.LatticePreconditioner(lat, s, noise, rank, factor_dtype=F32, true_diag=True)
        want = solvers.PivotedCholeskyPreconditioner(K.matmul, n, s, noise, rank, device=x.device, dtype=x.dtype,
                                                     true_diag=dk)
        Lg, Lw = got.L, want.L
        # the first pivot: p = argmax K_ii, and column 0 is s K e_p / sqrt(s K_pp)
        p = int(torch.argmax(dk))
        e = torch.zeros(n, 1, device="cuda")
        e[p] = 1.0
        col = s * K.matmul(e).reshape(-1) / float(s * dk[p]) ** 0.5
        scale = float(Lw.abs().max())
        assert float((Lg[:, 0] - col).abs().max()) <= 1e-5 * scale, "column 0 is the kernel row of argmax K_ii"
        assert float((Lg - Lw).abs().max()) <= 2e-4 * scale, float((Lg - Lw).abs().max()) / scale
        assert not torch.equal(Lg, ref.L), "the true diagonal changes the factor"
        # the float64 class passes the keyword through to the same fp32 factor
        if solvers._pcg_f64_available():
            got64 = solvers.LatticePreconditioner64(lat, s, noise, rank, true_diag=True)
            assert torch.equal(got64.L, Lg.double())
