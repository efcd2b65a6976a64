"""The one-sided fp32 position gradient of the rectangular product (plx_backward_splat_rows, plx_backward_contract_rows,
plx_apply_backward_rows) on the host: the C ABI's declarations and exports, the argument checks that need no built lattice and
return before any launch, the shape predicate at its edges, the dtype rule of Lattice.apply_backward_rows_f32, the switch,
the routing predicate's grad_f32 keyword, the dispatch of LatticeRowsProduct.backward on the positions' dtype, and the count
k32 of the bar."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice_kernel as lk
from tests.lattice64 import Lattice64, cloud
from tests.rows_backward32 import CASES, chunks32, depth64, k32
from tests.test_backward_f64_gpu import dkernel
from tests.test_rows_host import ROUTES

SYMBOLS = ("plx_backward_splat_rows", "plx_backward_contract_rows", "plx_apply_backward_rows")
PLX_ERR_INVALID = 1
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def bufs():
    """Six distinct 16-byte aligned host addresses: every call below returns before a launch could reach them, and before
    the lattice pointer (one of them) is followed."""
    raw = (ctypes.c_float * 1026)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    out = [ctypes.c_void_p(base + i * 128 * 4) for i in range(6)]
    out[0]._keep = raw
    return out


def test_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _native._SIGNATURES, name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert f" T {name}\n" in exported, name
    # the feature is detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_signatures():
    sig, vp, i64, i32 = _native._SIGNATURES, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    # (lat, a, a_begin, a_count, x, nrhs, values, stream)
    assert sig["plx_backward_splat_rows"] == (i32, [vp, vp, i64, i64, vp, i32, vp, vp])
    # (lat, values, b, b_begin, b_count, x, nrhs, grad_x, filtered, stream)
    assert sig["plx_backward_contract_rows"] == (i32, [vp, vp, vp, i64, i64, vp, i32, vp, vp, vp])
    # (lat, a, a_begin, a_count, b, b_begin, b_count, x, nrhs, grad_x, filtered, stream)
    assert sig["plx_apply_backward_rows"] == (i32, [vp, vp, i64, i64, vp, i64, i64, vp, i32, vp, vp, vp])


def _splat(lib, lat, a, x, values, nrhs=2, count=4):
    return lib.plx_backward_splat_rows(lat, a, 0, count, x, nrhs, values, None)


def _contract(lib, lat, values, b, x, gx, fl, nrhs=2, count=4):
    return lib.plx_backward_contract_rows(lat, values, b, 0, count, x, nrhs, gx, fl, None)


def _apply(lib, lat, a, b, x, gx, fl, nrhs=2, a_count=4, b_count=4):
    return lib.plx_apply_backward_rows(lat, a, 0, a_count, b, 4, b_count, x, nrhs, gx, fl, None)


def test_argument_checks_return_before_any_launch(lib, bufs):
    """Every PLX_ERR_INVALID that needs no built lattice, on host addresses: the lattice pointer is never followed and a
    launch that followed any of these would fault."""
    lat, a, b, x, o1, o2 = bufs
    err = lib.plx_last_error
    # a NULL lattice
    assert _splat(lib, None, a, x, o1) == PLX_ERR_INVALID and b"NULL" in err()
    assert _contract(lib, None, o1, b, x, o2, None) == PLX_ERR_INVALID and b"NULL" in err()
    assert _apply(lib, None, a, b, x, o1, o2) == PLX_ERR_INVALID and b"NULL" in err()
    # NULL buffers, one at a time; d_filtered alone may be NULL, so that call gets past the NULL test to the next refusal
    for i in range(3):
        args = [a, x, o1]
        args[i] = None
        assert _splat(lib, lat, *args) == PLX_ERR_INVALID and b"plx_backward_splat_rows: NULL" in err(), i
    for i in range(4):
        args = [o1, b, x, o2]
        args[i] = None
        assert _contract(lib, lat, *args, None) == PLX_ERR_INVALID and b"plx_backward_contract_rows: NULL" in err(), i
    for i in range(4):
        args = [a, b, x, o1]
        args[i] = None
        assert _apply(lib, lat, *args, None) == PLX_ERR_INVALID and b"plx_apply_backward_rows: NULL" in err(), i
    assert _apply(lib, lat, a, b, x, o1, None, nrhs=0) == PLX_ERR_INVALID and b"positive" in err()
    # nrhs < 1
    for nrhs in (0, -3):
        assert _splat(lib, lat, a, x, o1, nrhs=nrhs) == PLX_ERR_INVALID and b"nrhs" in err()
        assert _contract(lib, lat, o1, b, x, o2, None, nrhs=nrhs) == PLX_ERR_INVALID and b"nrhs" in err()
        assert _apply(lib, lat, a, b, x, o1, o2, nrhs=nrhs) == PLX_ERR_INVALID and b"nrhs" in err()
    # a count < 1
    for count in (0, -2):
        assert _splat(lib, lat, a, x, o1, count=count) == PLX_ERR_INVALID and b"row count" in err()
        assert _contract(lib, lat, o1, b, x, o2, None, count=count) == PLX_ERR_INVALID and b"row count" in err()
        assert _apply(lib, lat, a, b, x, o1, o2, a_count=count) == PLX_ERR_INVALID and b"row count" in err()
        assert _apply(lib, lat, a, b, x, o1, o2, b_count=count) == PLX_ERR_INVALID and b"row count" in err()
    # outputs aliasing inputs or each other
    for inp in (a, x):
        assert _splat(lib, lat, a, x, inp) == PLX_ERR_INVALID and b"alias" in err()
    for inp in (a, b, x):
        assert _apply(lib, lat, a, b, x, inp, None) == PLX_ERR_INVALID and b"alias" in err()
        assert _apply(lib, lat, a, b, x, o1, inp) == PLX_ERR_INVALID and b"alias" in err()
    for inp in (o1, b, x):
        assert _contract(lib, lat, o1, b, x, inp, None) == PLX_ERR_INVALID and b"alias" in err()
        assert _contract(lib, lat, o1, b, x, o2, inp) == PLX_ERR_INVALID and b"alias" in err()
    assert _apply(lib, lat, a, b, x, o1, o1) == PLX_ERR_INVALID and b"alias" in err()
    assert _contract(lib, lat, o1, b, x, o2, o2) == PLX_ERR_INVALID and b"alias" in err()
    # (d_values off 16-byte alignment, a range outside [0, n) and the column limit need a built lattice:
    # tests/test_rows_backward_gpu.py)


def test_backward_rows_ok_at_its_edges():
    ok = plx.Lattice.backward_rows_ok
    assert plx.Lattice.BACKWARD_ROWS_MAX_STRIDE == 4096
    assert ok(1, 1) is True                            # H = 2, the smallest row
    assert ok(512, 7) is True                          # H = 4096 exactly
    assert ok(2048, 1) is True
    assert ok(2049, 1) is False                        # H = 4098 rounds up to 4100
    assert ok(513, 7) is False                         # 4104
    assert ok(4093, 0) is False                        # d < 1, whatever the width
    assert ok(1, 4092) is True and ok(1, 4095) is True and ok(1, 4096) is False       # H = 4093 and 4096; 4097 rounds to 4100
    assert not ok(0, 8) and not ok(-1, 8) and not ok(8, 0) and not ok(8, -1)
    # the float64 predicates are where they were
    assert plx.Lattice.backward_rows_f64_ok(256, 7) and not plx.Lattice.backward_rows_f64_ok(257, 7)
    assert plx.Lattice.backward_f64_ok(128, 7) and not plx.Lattice.backward_f64_ok(129, 7)


def test_apply_backward_rows_f32_takes_float32_only():
    """Any float64 tensor among the three is refused by the dtypes before anything else is looked at -- wherever the tensors
    live, so no lattice has to be built for it."""
    lat = object.__new__(plx.Lattice)                  # no handle: the dtype rule comes before any use of it
    t64 = lambda *s: torch.randn(*s, dtype=F64)        # noqa: E731
    t32 = lambda *s: torch.randn(*s)                   # noqa: E731
    for mask in range(1, 8):                           # every combination with a float64 tensor in it; 7 is all-fp64
        a, b, x = ((t64 if mask >> i & 1 else t32)(6, k) for i, k in enumerate((2, 2, 3)))
        for want in (True, False):
            with pytest.raises(TypeError, match="float32"):
                lat.apply_backward_rows_f32(a, 0, b, 0, x, want_filtered=want)
    with pytest.raises(TypeError):
        lat.apply_backward_rows_f32([[0.0]], 0, t32(1, 1), 0, t32(1, 1))
    with pytest.raises(ValueError, match="no CPU path"):
        lat.apply_backward_rows_f32(t32(6, 2), 0, t32(6, 2), 0, t32(6, 3))
    # the float64 method still refuses every float32 tensor
    with pytest.raises(TypeError, match="no fp32 form"):
        lat.apply_backward_rows(t32(6, 2), 0, t32(6, 2), 0, t32(6, 3))


def test_the_switch_exists_and_is_off():
    assert plx.RectangularLazyLattice.native_rows_grad is False
    assert plx.RectangularLazyLattice.native_rows_grad_f64 is False
    assert plx.RectangularLazyLattice.native_rows is True and plx.RectangularLazyLattice.native_min_columns == 101
    assert callable(plx.Lattice.apply_backward_rows_f32)


@pytest.mark.parametrize("device,dtype,dim,hook,grad,enabled,want", ROUTES)
def test_routing_predicate_without_the_keyword_is_unchanged(device, dtype, dim, hook, grad, enabled, want):
    assert lk.rows_route(device, dtype, dim, hook, grad, enabled) is want
    assert lk.rows_route(device, dtype, dim, hook, grad, enabled, grad_f32=False) is want
    for f64 in (False, True):
        for grad_f64 in (False, True):
            assert lk.rows_route(device, dtype, dim, hook, grad, enabled, f64=f64, grad_f64=grad_f64) is \
                lk.rows_route(device, dtype, dim, hook, grad, enabled, f64=f64, grad_f64=grad_f64, grad_f32=False)
    # grad_f64 with float32 stays False
    assert lk.rows_route(device, F32, dim, hook, grad, enabled, grad_f64=True) is False
    # with the keyword: only a CUDA float32 2-D right-hand side whose positions want a gradient, no hook, the route on
    got = lk.rows_route(device, dtype, dim, hook, grad, enabled, grad_f32=True)
    assert got is False if dtype != F32 else got is ((device, dim, hook, grad, enabled) == ("cuda", 2, None, True, True))
    got32 = lk.rows_route(device, F32, dim, hook, grad, enabled, grad_f32=True)
    assert got32 is ((device, dim, hook, grad, enabled) == ("cuda", 2, None, True, True))


def test_routing_predicate_with_the_grad_keyword():
    assert lk.rows_route("cuda", F32, 2, None, True, grad_f32=True) is True
    assert lk.rows_route("cuda", F32, 2, None, True, True, 1, 101, grad_f32=True) is True     # no width gate
    assert lk.rows_route("cuda", F32, 2, None, False, grad_f32=True) is False                 # nothing wants a gradient
    assert lk.rows_route("cuda", F64, 2, None, True, grad_f32=True) is False                  # the float64 form has its own
    assert lk.rows_route("cuda", F64, 2, None, True, f64=True, grad_f32=True) is False
    assert lk.rows_route("cuda", torch.float16, 2, None, True, grad_f32=True) is False
    assert lk.rows_route("cpu", F32, 2, None, True, grad_f32=True) is False
    assert lk.rows_route("cuda", F32, 3, None, True, grad_f32=True) is False
    assert lk.rows_route("cuda", F32, 2, object(), True, grad_f32=True) is False
    assert lk.rows_route("cuda", F32, 2, None, True, False, grad_f32=True) is False
    # without it a wanted gradient refuses, as before
    assert lk.rows_route("cuda", F32, 2, None, True) is False
    assert lk.rows_route("cuda", F32, 2, None, True, grad_f64=True) is False


class _StubLattice:
    """Records which one-sided method LatticeRowsProduct.backward calls."""

    def __init__(self, d):
        self.d, self.calls = d, []

    def _one(self, name, a, b, x, want_filtered):
        self.calls.append((name, a.dtype, b.dtype, x.dtype, want_filtered))
        return torch.zeros((b.shape[0], self.d), dtype=x.dtype), (torch.zeros_like(b) if want_filtered else None)

    def apply_backward_rows(self, a, a_begin, b, b_begin, x, want_filtered=True):
        return self._one("f64", a, b, x, want_filtered)

    def apply_backward_rows_f32(self, a, a_begin, b, b_begin, x, want_filtered=True):
        return self._one("f32", a, b, x, want_filtered)


class _Ctx:
    pass


@pytest.mark.parametrize("dtype,name", [(F32, "f32"), (F64, "f64")])
def test_backward_calls_the_method_of_the_positions_dtype(monkeypatch, dtype, name):
    n, d, L, sc = 7, 3, 2, 4
    stub = _StubLattice(d)
    monkeypatch.setattr(lk._cache, "get", lambda positions, coeffs: stub)
    ctx = _Ctx()
    ctx.ranges, ctx.deriv_coeffs, ctx.needs_input_grad = (0, sc, sc, n - sc), object(), (True, True)
    ctx.saved_tensors = (torch.ones(sc, L, dtype=dtype), torch.ones(n, d, dtype=dtype))
    out = lk.LatticeRowsProduct.backward(ctx, torch.ones(n - sc, L, dtype=dtype))
    assert [c[0] for c in stub.calls] == [name, name]
    assert all(c[1:4] == (dtype,) * 3 for c in stub.calls) and [c[4] for c in stub.calls] == [True, False]
    grad_source, grad_positions = out[0], out[1]
    assert grad_source.shape == (sc, L) and grad_positions.shape == (n, d) and grad_positions.dtype == dtype
    assert all(o is None for o in out[2:])


def test_k32_and_the_case_list():
    """k32 against its formula on a small CPU lattice, and the case list against the chunk boundaries it was chosen at."""
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    x = cloud("gauss1", 101, 3, seed=2, coeffs=dtaps).astype(np.float64)
    l64 = Lattice64(x, dtaps)
    lmax = int(np.diff(l64.S.tocsc().indptr).max())
    d, r = 3, dtaps.size // 2
    assert k32(l64) == 2 * lmax + 2 * (2 * r + 1) * (d + 1) + 3 * (d + 1) + 9
    # every operation depth64 counts once is counted at least twice here, but for its slack
    assert k32(l64) >= 2 * (depth64(l64) - 8)
    shapes = {(d, L): chunks32(d, L) for d, L, *_ in CASES}
    assert shapes == {(1, 1): 1, (8, 1): 3, (8, 3): 7, (3, 2): 2, (8, 11): 25, (3, 64): 64, (5, 43): 65, (9, 26): 65,
                      (18, 1): 5, (18, 16): 76, (24, 1): 7, (24, 11): 69}
    assert {o for _, _, o, *_ in CASES} == {0, 1, 2, 3} and {p for _, _, _, p, *_ in CASES} == {"rbf", "matern32"}
    assert {a for *_, a, _ in CASES} == {True, False}
    for d, L, *_ in CASES:
        assert plx.Lattice.backward_rows_ok(L, d)
