"""The position gradient of a query (plx_slice_at_dots, plx_slice_at_dots_f64, plx_locate_pullback,
plx_locate_pullback_f64) on the host: the C ABI's declarations and exports, the refusals that need no lattice, LatticeQuery's
sixth field, the argument rules of query_grad.slice_at_dots / locate_pullback / slice_at_backward, LatticeSliceAt's refusal of a
`values` that wants a gradient, and PredictionCache.predict_query_grad off the query route.
Fails without the feature."""
import ctypes
import functools
import re
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice as lattice_mod
from simplex_gp_amd import lattice_kernel, query_grad, training
from tests.test_query_host import _cache, _CudaLike, _NoHandle

SYMBOLS = {"plx_slice_at_dots": 8, "plx_slice_at_dots_f64": 8, "plx_locate_pullback": 6, "plx_locate_pullback_f64": 6}
PLX_ERR_INVALID = 1
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def test_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(_native.HEADER_PATH).read(), flags=re.S)
    declared = _native.declared_symbols()
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name, arity in SYMBOLS.items():
        assert name in declared and name in _native._SIGNATURES and name in _native.OPTIONAL_SYMBOLS, name
        assert hasattr(lib, name), name
        assert f" T {name}\n" in exported, name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(_native._SIGNATURES[name][1]), name
    # detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_signatures():
    sig, vp, i64, i32 = _native._SIGNATURES, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert sig["plx_slice_at_dots"] == sig["plx_slice_at_dots_f64"] == sig["plx_slice_at"] == (i32, [vp, vp, i32, vp, vp, i64, vp, vp])
    assert sig["plx_locate_pullback"] == sig["plx_locate_pullback_f64"] == (i32, [vp, vp, vp, i64, vp, vp])


def test_a_null_lattice_is_refused(lib):
    """PLX_ERR_INVALID before the lattice pointer is followed or anything is launched: the buffers are host addresses,
    sentinel-filled, and stay as they were."""
    raw = (ctypes.c_float * 256)(*([7.0] * 256))
    base = ctypes.addressof(raw)
    base += (-base) % 16
    a, b, c, e = (ctypes.c_void_p(base + 128 * i) for i in range(4))
    err = lib.plx_last_error
    assert lib.plx_slice_at_dots(None, a, 2, b, c, 4, e, None) == PLX_ERR_INVALID and b"plx_slice_at_dots" in err()
    assert lib.plx_slice_at_dots_f64(None, a, 2, b, c, 4, e, None) == PLX_ERR_INVALID and b"plx_slice_at_dots_f64" in err()
    assert lib.plx_locate_pullback(None, a, b, 4, c, None) == PLX_ERR_INVALID and b"plx_locate_pullback" in err()
    assert lib.plx_locate_pullback_f64(None, a, b, 4, c, None) == PLX_ERR_INVALID and b"plx_locate_pullback_f64" in err()
    assert all(v == 7.0 for v in raw)


def _query(nq, d, build_id=1, x=True):
    args = (torch.zeros((d + 1, nq), dtype=torch.int32), torch.zeros((d + 1, nq)), torch.zeros(nq), nq, build_id)
    return plx.lattice.LatticeQuery(*args, torch.zeros(nq, d)) if x else plx.lattice.LatticeQuery(*args)


def test_lattice_query_keeps_its_five_argument_form():
    q5 = _query(4, 2, build_id=5, x=False)
    assert q5.x is None and (q5.nq, q5.build_id) == (4, 5) and tuple(q5.vid.shape) == tuple(q5.weight.shape) == (3, 4)
    q6 = _query(4, 2, build_id=5)
    assert tuple(q6.x.shape) == (4, 2) and q6.x.dtype == F32
    qk = plx.lattice.LatticeQuery(q5.vid, q5.weight, q5.mass, 4, 5, x=q6.x)
    assert qk.x is q6.x
    for name in ("slice_at_dots", "locate_pullback", "slice_at_backward", "kernels"):
        assert callable(getattr(query_grad, name)), name
    assert plx.query_grad is query_grad
    assert issubclass(lattice_kernel.LatticeSliceAt, torch.autograd.Function)
    assert callable(training.PredictionCache.predict_query_grad)


def test_a_library_without_the_symbols_is_named(monkeypatch):
    lat = object.__new__(plx.Lattice)                  # no handle: the symbol is asked for before any use of it
    cl = lambda t: t.as_subclass(_CudaLike)
    g32, g64 = cl(torch.zeros(3, 4)), cl(torch.zeros(3, 4, dtype=F64))
    for missing, call in (("plx_slice_at_dots", lambda: query_grad.slice_at_dots(lat, cl(torch.zeros(3, 4)), _query(3, 1), g32)),
                          ("plx_slice_at_dots_f64", lambda: query_grad.slice_at_dots(lat, cl(torch.zeros(3, 4, dtype=F64)), _query(3, 1), g64)),
                          ("plx_locate_pullback", lambda: query_grad.slice_at_backward(lat, cl(torch.zeros(3, 4)), _query(3, 1), g32)),
                          ("plx_locate_pullback_f64",
                           lambda: query_grad.slice_at_backward(lat, cl(torch.zeros(3, 4, dtype=F64)), _query(3, 1), g64)),
                          ("plx_locate_pullback", lambda: query_grad.locate_pullback(lat, _query(3, 1), cl(torch.zeros(2, 3)))),
                          ("plx_locate_pullback_f64", lambda: query_grad.locate_pullback(lat, _query(3, 1), cl(torch.zeros(2, 3, dtype=F64)))),
                          ("plx_last_query_kernels", lambda: query_grad.kernels(lat))):
        monkeypatch.setattr(lattice_mod.nv, "has_symbols", lambda *names, _m=missing: _m not in names)
        with pytest.raises(RuntimeError, match=missing + r"\b"):
            call()


class _Stub:
    """A library that has every symbol and none of whose device calls may be reached: the argument rules come first.  The
    row strides (pure functions of vd) are the loaded library's."""

    def __init__(self, real):
        self.plx_values_stride, self.plx_values_stride_f64 = real.plx_values_stride, real.plx_values_stride_f64

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


@pytest.fixture
def stub(monkeypatch):
    stub_lib = _Stub(_native.lib())
    monkeypatch.setattr(lattice_mod.nv, "has_symbols", lambda *names: True)
    monkeypatch.setattr(lattice_mod.nv, "lib", lambda: stub_lib)


def test_slice_at_backward_argument_rules(stub):
    """The errors of slice_at, in its order, for all three calls of the gradient; then grad_out's own."""
    lat = _NoHandle()                                                      # d = 2, m = 5, build 3
    cl = lambda t: t.as_subclass(_CudaLike)
    q = _query(4, 2, build_id=3)
    g = cl(torch.zeros(4, 4))
    for fn in (functools.partial(query_grad.slice_at_backward, lat), functools.partial(query_grad.slice_at_dots, lat)):
        with pytest.raises(TypeError, match="LatticeQuery"):
            fn(cl(torch.zeros(5, 4)), (q.vid, q.weight), g)
        with pytest.raises(TypeError):
            fn([[0.0]], q, g)
        with pytest.raises(ValueError, match="CUDA"):
            fn(torch.zeros(5, 4), q, g)
        with pytest.raises(TypeError, match="float32 or float64"):
            fn(cl(torch.zeros(5, 4, dtype=torch.float16)), q, g)
        with pytest.raises(ValueError, match="2-D"):
            fn(cl(torch.zeros(20)), q, g)
        with pytest.raises(RuntimeError, match="rebuilt"):
            fn(cl(torch.zeros(5, 4)), _query(4, 2, build_id=2), g)
        with pytest.raises(TypeError, match="grad_out"):
            fn(cl(torch.zeros(5, 4)), q, cl(torch.zeros(4, 4, dtype=F64)))             # not the dtype of values
        with pytest.raises(TypeError, match="grad_out"):
            fn(cl(torch.zeros(5, 4)), q, [[0.0]])


def test_locate_pullback_argument_rules(stub):
    lat = _NoHandle()
    cl = lambda t: t.as_subclass(_CudaLike)
    q = _query(4, 2, build_id=3)
    with pytest.raises(TypeError, match="LatticeQuery"):
        query_grad.locate_pullback(lat, (q.vid, q.weight), cl(torch.zeros(3, 4)))
    with pytest.raises(ValueError, match="CUDA"):
        query_grad.locate_pullback(lat, q, torch.zeros(3, 4))
    with pytest.raises(TypeError, match="float32 or float64"):
        query_grad.locate_pullback(lat, q, cl(torch.zeros(3, 4, dtype=torch.float16)))
    with pytest.raises(RuntimeError, match="rebuilt"):
        query_grad.locate_pullback(lat, _query(4, 2, build_id=2), cl(torch.zeros(3, 4)))
    with pytest.raises(ValueError, match="positions"):
        query_grad.locate_pullback(lat, _query(4, 2, build_id=3, x=False), cl(torch.zeros(3, 4)))    # a five-argument query
    with pytest.raises(ValueError, match=r"\[3, 4\]"):
        query_grad.locate_pullback(lat, q, cl(torch.zeros(4, 3)))                                    # t is [d + 1, nq]


def test_slice_at_refuses_values_that_want_a_gradient():
    """Before anything is located: the lattice is never touched."""
    x = torch.zeros(4, 2, requires_grad=True)
    values = torch.zeros(5, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="adjoint splat at query points is not built"):
        lattice_kernel.LatticeSliceAt.apply(x, values, object(), 4)


def test_predict_query_grad_raises_off_the_query_route():
    """A host model: _query_state() is None, predict(route="query") falls through, predict_query_grad raises."""
    c = _cache()
    assert c._query_state() is None
    with pytest.raises(RuntimeError, match="query route"):
        c.predict_query_grad(torch.zeros(4, 2, requires_grad=True))
    assert c.model.log == []
