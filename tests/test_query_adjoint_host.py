"""The splat at query points (plx_query_plan_bytes, plx_query_plan, plx_splat_at, plx_splat_at_f64,
plx_last_splat_at_kernels) on the host: the C ABI's declarations and exports, the refusals that need no lattice, the
missing-symbol errors and the argument rules of query_adjoint.plan / splat_at / slice_at_adjoint / apply_at_t.
Fails without the feature."""
import ctypes
import re
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice as lattice_mod
from simplex_gp_amd import lattice_kernel, query_adjoint
from tests.test_query_host import _CudaLike, _NoHandle

SYMBOLS = {"plx_query_plan_bytes": 2, "plx_query_plan": 6, "plx_splat_at": 7, "plx_splat_at_f64": 7,
           "plx_last_splat_at_kernels": 3}
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
    assert sig["plx_query_plan_bytes"] == (i64, [vp, i64])
    assert sig["plx_query_plan"] == (i32, [vp, vp, vp, i64, vp, vp])
    assert sig["plx_splat_at"] == sig["plx_splat_at_f64"] == (i32, [vp, vp, vp, i32, i64, vp, vp])
    assert sig["plx_last_splat_at_kernels"] == sig["plx_last_query_kernels"] == (i32, [vp, ctypes.c_char_p, i32])


def test_a_null_lattice_is_refused(lib):
    """-1 / PLX_ERR_INVALID before the lattice pointer is followed or anything is launched: the buffers are host
    addresses, sentinel-filled, and stay as they were."""
    assert lib.plx_query_plan_bytes(None, 5) == -1
    raw = (ctypes.c_float * 256)(*([7.0] * 256))
    base = ctypes.addressof(raw)
    base += (-base) % 16
    a, b, c = (ctypes.c_void_p(base + 256 * i) for i in range(3))
    err = lib.plx_last_error
    assert lib.plx_query_plan(None, a, b, 4, c, None) == PLX_ERR_INVALID and b"plx_query_plan" in err()
    assert lib.plx_splat_at(None, a, b, 2, 4, c, None) == PLX_ERR_INVALID and b"plx_splat_at" in err()
    assert lib.plx_splat_at_f64(None, a, b, 2, 4, c, None) == PLX_ERR_INVALID and b"plx_splat_at_f64" in err()
    buf = ctypes.create_string_buffer(16)
    assert lib.plx_last_splat_at_kernels(None, buf, 16) == PLX_ERR_INVALID
    assert all(v == 7.0 for v in raw)


def _query(nq, d, build_id=3):
    return plx.lattice.LatticeQuery(torch.zeros((d + 1, nq), dtype=torch.int32), torch.zeros((d + 1, nq)), torch.zeros(nq), nq,
                                    build_id, torch.zeros(nq, d))


def _plan(nq, build_id=3):
    return query_adjoint.QueryPlan(torch.zeros(64, dtype=torch.uint8), nq, build_id)


def test_the_module_and_the_functions_exist():
    for name in ("QueryPlan", "plan", "splat_at", "slice_at_adjoint", "apply_at_t", "kernels"):
        assert callable(getattr(query_adjoint, name)), name
    assert plx.query_adjoint is query_adjoint
    p = _plan(4, build_id=5)
    assert (p.nq, p.build_id) == (4, 5) and p.buffer.dtype == torch.uint8
    for cls in (lattice_kernel.LatticeSliceAtValues, lattice_kernel.LatticeQueryProduct):
        assert issubclass(cls, torch.autograd.Function)
    # none of it is a method of Lattice: the interleave table does not list these ops
    for name in ("splat_at", "plan", "apply_at_t", "slice_at_adjoint"):
        assert not hasattr(plx.Lattice, name), name


def test_a_library_without_the_symbols_is_named(monkeypatch):
    lat = object.__new__(plx.Lattice)                  # no handle: the symbol is asked for before any use of it
    cl = lambda t: t.as_subclass(_CudaLike)
    g32, g64 = cl(torch.zeros(3, 4)), cl(torch.zeros(3, 4, dtype=F64))
    q = _query(3, 1)
    for missing, call in (("plx_query_plan_bytes", lambda: query_adjoint.plan(lat, q)),
                          ("plx_query_plan", lambda: query_adjoint.plan(lat, q)),
                          ("plx_query_plan", lambda: query_adjoint.splat_at(lat, g32, q)),
                          ("plx_splat_at", lambda: query_adjoint.splat_at(lat, g32, q, plan=_plan(3))),
                          ("plx_splat_at_f64", lambda: query_adjoint.splat_at(lat, g64, q, plan=_plan(3))),
                          ("plx_splat_at", lambda: query_adjoint.slice_at_adjoint(lat, g32, q)),
                          ("plx_splat_at_f64", lambda: query_adjoint.apply_at_t(lat, g64, q)),
                          ("plx_last_splat_at_kernels", lambda: query_adjoint.kernels(lat))):
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


def test_argument_rules(stub):
    """Type, device and shape errors as slice_at_dots raises them; the stale build and the foreign plan raise "rebuilt"."""
    lat = _NoHandle()                                                      # d = 2, m = 5, build 3
    cl = lambda t: t.as_subclass(_CudaLike)
    q = _query(4, 2)
    g = cl(torch.zeros(4, 3))
    for fn in (query_adjoint.splat_at, query_adjoint.slice_at_adjoint, query_adjoint.apply_at_t):
        with pytest.raises(TypeError):
            fn(lat, [[0.0]], q, plan=_plan(4))
        with pytest.raises(ValueError, match="CUDA"):
            fn(lat, torch.zeros(4, 3), q, plan=_plan(4))
        with pytest.raises(TypeError, match="float32 or float64"):
            fn(lat, cl(torch.zeros(4, 3, dtype=torch.float16)), q, plan=_plan(4))
        with pytest.raises(ValueError, match="2-D"):
            fn(lat, cl(torch.zeros(12)), q, plan=_plan(4))
        with pytest.raises(TypeError, match="LatticeQuery"):
            fn(lat, g, (q.vid, q.weight), plan=_plan(4))
        with pytest.raises(RuntimeError, match="rebuilt"):
            fn(lat, g, _query(4, 2, build_id=2), plan=_plan(4))
        with pytest.raises(ValueError, match=r"\[4, vd >= 1\]"):
            fn(lat, cl(torch.zeros(5, 3)), q, plan=_plan(4))               # not nq rows
        with pytest.raises(TypeError, match="QueryPlan"):
            fn(lat, g, q, plan=torch.zeros(8))
        with pytest.raises(RuntimeError, match="rebuilt"):
            fn(lat, g, q, plan=_plan(4, build_id=2))                       # the plan of another build
        with pytest.raises(RuntimeError, match="rebuilt"):
            fn(lat, g, q, plan=_plan(5))                                   # the plan of another nq
    with pytest.raises(TypeError, match="values"):
        query_adjoint.splat_at(lat, g, q, plan=_plan(4), values=cl(torch.zeros(5, 4, dtype=F64)))
    with pytest.raises(ValueError, match=r"\[5, 4\]"):
        query_adjoint.splat_at(lat, g, q, plan=_plan(4), values=cl(torch.zeros(5, 3)))
    with pytest.raises(TypeError, match="LatticeQuery"):
        query_adjoint.plan(lat, (q.vid, q.weight))
    with pytest.raises(RuntimeError, match="rebuilt"):
        query_adjoint.plan(lat, _query(4, 2, build_id=2))
