"""Queries at points that are not the build's (plx_locate, plx_slice_at, plx_slice_at_f64, plx_last_query_kernels) on the
host: the C ABI's declarations and exports, the refusals that need no lattice, the argument rules of Lattice.locate /
Lattice.slice_at, the switch, and the routing of PredictionCache.predict with the switch off (what it called before).
Fails without the feature."""
import ctypes
import re
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice as lattice_mod
from simplex_gp_amd import training

SYMBOLS = {"plx_locate": 7, "plx_slice_at": 8, "plx_slice_at_f64": 8, "plx_last_query_kernels": 3}
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
    assert sig["plx_locate"] == (i32, [vp, vp, i64, vp, vp, vp, vp])
    assert sig["plx_slice_at"] == sig["plx_slice_at_f64"] == (i32, [vp, vp, i32, vp, vp, i64, vp, vp])
    assert sig["plx_last_query_kernels"] == sig["plx_last_kernels"] == (i32, [vp, ctypes.c_char_p, i32])


def test_a_null_lattice_is_refused(lib):
    """PLX_ERR_INVALID before the lattice pointer is followed or anything is launched: the buffers are host addresses,
    sentinel-filled, and stay as they were."""
    raw = (ctypes.c_float * 256)(*([7.0] * 256))
    base = ctypes.addressof(raw)
    base += (-base) % 16
    a, b, c, e = (ctypes.c_void_p(base + 128 * i) for i in range(4))
    err = lib.plx_last_error
    assert lib.plx_locate(None, a, 4, b, c, e, None) == PLX_ERR_INVALID and b"plx_locate" in err()
    assert lib.plx_locate(None, a, 4, b, c, None, None) == PLX_ERR_INVALID and b"plx_locate" in err()
    assert lib.plx_slice_at(None, a, 2, b, c, 4, e, None) == PLX_ERR_INVALID and b"plx_slice_at" in err()
    assert lib.plx_slice_at_f64(None, a, 2, b, c, 4, e, None) == PLX_ERR_INVALID and b"plx_slice_at_f64" in err()
    assert lib.plx_last_query_kernels(None, ctypes.create_string_buffer(8), 8) == PLX_ERR_INVALID
    assert all(v == 7.0 for v in raw)


def test_a_library_without_the_symbols_is_named(monkeypatch):
    lat = object.__new__(plx.Lattice)                  # no handle: the symbol is asked for before any use of it
    cl = lambda t: t.as_subclass(_CudaLike)
    for missing, call in (("plx_locate", lambda: lat.locate(cl(torch.zeros(3, 2)))),
                          ("plx_slice_at", lambda: lat.slice_at(cl(torch.zeros(3, 4)), _query(3, 1))),
                          ("plx_slice_at_f64", lambda: lat.slice_at(cl(torch.zeros(3, 4, dtype=F64)), _query(3, 1))),
                          ("plx_last_query_kernels", lambda: lat.query_kernels())):
        monkeypatch.setattr(lattice_mod.nv, "has_symbols", lambda *names, _m=missing: _m not in names)
        with pytest.raises(RuntimeError, match=missing + r"\b"):
            call()


def _query(nq, d, build_id=1):
    return plx.lattice.LatticeQuery(torch.zeros((d + 1, nq), dtype=torch.int32), torch.zeros((d + 1, nq)), torch.zeros(nq),
                                    nq, build_id)


class _CudaLike(torch.Tensor):
    """A host tensor that says it is on the device: enough for the argument rules that come before any device work."""
    is_cuda = property(lambda self: True)


class _NoHandle(plx.Lattice):
    """A Lattice without a native handle: d, m and the build id are what the argument rules compare against."""
    d, m, n, build_id = 2, 5, 9, 3
    device = torch.device("cpu")

    def __init__(self):
        pass

    def __del__(self):
        pass


def test_locate_argument_rules():
    lat = _NoHandle()
    with pytest.raises(TypeError):
        lat.locate([[0.0, 0.0]])                                       # not a tensor
    with pytest.raises(ValueError, match="CUDA"):
        lat.locate(torch.zeros(4, 2))                                  # a host tensor
    for dtype in (torch.float16, torch.int32, torch.bfloat16):
        with pytest.raises(TypeError, match="float32"):
            lat.locate(torch.zeros(4, 2, dtype=dtype).as_subclass(_CudaLike))
    with pytest.raises(ValueError, match="2-D"):
        lat.locate(torch.zeros(4).as_subclass(_CudaLike))
    with pytest.raises(ValueError, match=r"\[nq >= 1, 2\]"):
        lat.locate(torch.zeros(4, 3).as_subclass(_CudaLike))          # d of the lattice is 2
    with pytest.raises(ValueError, match=r"\[nq >= 1, 2\]"):
        lat.locate(torch.zeros(0, 2).as_subclass(_CudaLike))
    with pytest.raises(ValueError, match=r"\[nq >= 1, 2\]"):
        lat.locate(torch.zeros(4, 3, dtype=F64).as_subclass(_CudaLike))    # float64 is rounded, then held to the same shape


def test_slice_at_argument_rules():
    lat = _NoHandle()
    cl = lambda t: t.as_subclass(_CudaLike)
    q = _query(4, 2, build_id=3)
    with pytest.raises(TypeError, match="LatticeQuery"):
        lat.slice_at(cl(torch.zeros(5, 4)), (q.vid, q.weight))
    with pytest.raises(TypeError):
        lat.slice_at([[0.0]], q)
    with pytest.raises(ValueError, match="CUDA"):
        lat.slice_at(torch.zeros(5, 4), q)
    with pytest.raises(TypeError, match="float32 or float64"):
        lat.slice_at(cl(torch.zeros(5, 4, dtype=torch.float16)), q)
    with pytest.raises(ValueError, match="2-D"):
        lat.slice_at(cl(torch.zeros(20)), q)
    # a location of another build: refused by the build id, before any device work
    with pytest.raises(RuntimeError, match="rebuilt"):
        lat.slice_at(cl(torch.zeros(5, 4)), _query(4, 2, build_id=2))


def test_lattice_query_holds_what_the_issue_names():
    q = _query(4, 2, build_id=5)
    assert (q.nq, q.build_id) == (4, 5) and q.vid.dtype == torch.int32 and q.weight.dtype == F32 and q.mass.dtype == F32
    assert tuple(q.vid.shape) == tuple(q.weight.shape) == (3, 4) and tuple(q.mass.shape) == (4,)
    for name in ("locate", "slice_at", "blurred", "apply_at", "query_kernels"):
        assert callable(getattr(plx.Lattice, name)), name


# ---- the model layer ----------------------------------------------------------------------------------------------------
def test_the_switch_exists_and_is_off():
    assert training.PredictionCache.query_route is False


class _StubOperator:
    def __init__(self, log, tag, rows):
        self.log, self.tag, self.rows = log, tag, rows

    def matmul(self, V):
        self.log.append((self.tag, tuple(V.shape)))
        return torch.ones(self.rows, V.shape[1])


class _StubModel:
    """What PredictionCache.predict asks of the model on the stacked route: kernel(x*, x) -> an operator with matmul,
    kernel(x*, x*, diag=True), mean, outputscale."""
    mean, outputscale = torch.tensor(0.5), torch.tensor(2.0)

    def __init__(self):
        self.log = []

    def kernel(self, a, b, diag=False):
        if diag:
            self.log.append(("diag", a.shape[0]))
            return torch.ones(a.shape[0])
        return _StubOperator(self.log, "K_star", a.shape[0])


def _cache(variance=True):
    c = object.__new__(training.PredictionCache)
    c.model, c.x = _StubModel(), torch.zeros(6, 2)
    c.alpha = torch.ones(6, 1)
    c.Q = torch.ones(6, 3) if variance else None
    c.chol = torch.eye(3) if variance else None
    return c


@pytest.mark.parametrize("route", [None, "stacked", "query"])
def test_predict_routes_to_the_stacked_operator(route):
    """The default and route="stacked" call what predict called before: one rectangular product of [alpha, Q], the prior's
    diagonal, the formulas of the parent.  route="query" on a host model falls through to the same."""
    c = _cache()
    x_star = torch.zeros(4, 2)
    mean, var = c.predict(x_star) if route is None else c.predict(x_star, route=route)
    assert c.model.log == [("K_star", (6, 4)), ("diag", 4)]
    KAQ = 2.0 * torch.ones(4, 4)
    want_mean = 0.5 + KAQ[:, 0]
    want_var = (2.0 * torch.ones(4) - (torch.linalg.solve_triangular(torch.eye(3), KAQ[:, 1:].t(), upper=False) ** 2).sum(0)
                ).clamp_min(1e-8)
    assert torch.equal(mean, want_mean) and torch.equal(var, want_var)
    assert c.last_query_mass is None
    c2 = _cache(variance=False)
    mean, var = c2.predict(x_star, route=route)
    assert var is None and torch.equal(mean, 0.5 + 2.0 * torch.ones(4)) and c2.model.log == [("K_star", (6, 1))]


def test_an_unknown_route_is_refused():
    with pytest.raises(ValueError, match="route"):
        _cache().predict(torch.zeros(4, 2), route="fast")


def test_the_module_functions_pass_route_through(monkeypatch):
    seen = []

    class _C:
        def predict(self, x_star, route=None):
            seen.append(route)
            return torch.zeros(3), torch.ones(3)

    model = _StubModel()
    model.noise = torch.tensor(0.1)
    training.predict(model, None, None, torch.zeros(3, 2), cache=_C())
    training.predict(model, None, None, torch.zeros(3, 2), cache=_C(), route="query")
    training.evaluate(model, None, None, torch.zeros(3, 2), torch.zeros(3), cache=_C(), route="stacked")
    assert seen == [None, "query", "stacked"]
