"""The float64 rectangular product (plx_splat_rows_f64 / plx_slice_rows_f64 / plx_apply_rows_f64) on the host: the C ABI's
declarations and exports, the argument checks that return before any launch, the routing predicate's f64 keyword, and the
dtype rules of Lattice.apply_rows that need no GPU."""
import ctypes
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice_kernel as lk
from tests.test_rows_host import ROUTES

ROWS_F64_SYMBOLS = ("plx_splat_rows_f64", "plx_slice_rows_f64", "plx_apply_rows_f64", "plx_last_rows_f64_kernels")
PLX_ERR_INVALID = 1
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_double * 1024)()                  # host memory: every call below returns before a launch could reach it
    p = ctypes.cast(buf, ctypes.c_void_p)
    p._keep = buf
    return p


def test_rows_f64_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in ROWS_F64_SYMBOLS:
        assert name in declared and name in _native._SIGNATURES, name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in ROWS_F64_SYMBOLS:
        assert f" T {name}\n" in exported, name
    # the feature is detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_rows_f64_signatures_mirror_the_fp32_rows_calls():
    for name in ("plx_splat_rows", "plx_slice_rows", "plx_apply_rows"):
        assert _native._SIGNATURES[name + "_f64"] == _native._SIGNATURES[name], name
    assert _native._SIGNATURES["plx_last_rows_f64_kernels"] == _native._SIGNATURES["plx_last_rows_kernels"]


def test_rows_f64_argument_checks_return_before_any_launch(lib, p):
    # a NULL lattice, and NULL buffers next to a lattice pointer that is never followed (the NULL test comes first)
    for rc in (lib.plx_splat_rows_f64(None, p, 0, 4, 1, p, None), lib.plx_splat_rows_f64(p, None, 0, 4, 1, p, None),
               lib.plx_splat_rows_f64(p, p, 0, 4, 1, None, None)):
        assert rc == PLX_ERR_INVALID and b"plx_splat_rows_f64" in lib.plx_last_error() and b"NULL" in lib.plx_last_error()
    for rc in (lib.plx_slice_rows_f64(None, p, 1, 0, 4, p, None), lib.plx_slice_rows_f64(p, None, 1, 0, 4, p, None),
               lib.plx_slice_rows_f64(p, p, 1, 0, 4, None, None)):
        assert rc == PLX_ERR_INVALID and b"plx_slice_rows_f64" in lib.plx_last_error() and b"NULL" in lib.plx_last_error()
    for rc in (lib.plx_apply_rows_f64(None, p, 0, 4, 1, p, 4, 4, None), lib.plx_apply_rows_f64(p, None, 0, 4, 1, p, 4, 4, None),
               lib.plx_apply_rows_f64(p, p, 0, 4, 1, None, 4, 4, None)):
        assert rc == PLX_ERR_INVALID and b"plx_apply_rows_f64" in lib.plx_last_error() and b"NULL" in lib.plx_last_error()
    buf = ctypes.create_string_buffer(64)
    for rc in (lib.plx_last_rows_f64_kernels(None, buf, 64), lib.plx_last_rows_f64_kernels(p, None, 64),
               lib.plx_last_rows_f64_kernels(p, buf, 0)):
        assert rc == PLX_ERR_INVALID and b"plx_last_rows_f64_kernels" in lib.plx_last_error()


def test_routing_predicate_with_the_f64_keyword():
    assert lk.rows_route("cuda", F64, 2, None, False, f64=True) is True
    assert lk.rows_route("cuda", F64, 2, None, False, True, 101, 101, f64=True) is True
    assert lk.rows_route("cuda", F64, 2, None, False, True, 100, 101, f64=True) is False
    assert lk.rows_route("cuda", F64, 2, None, False) is False                   # without the keyword: as before
    assert lk.rows_route("cuda", F64, 2, None, False, f64=False) is False
    assert lk.rows_route("cuda", F32, 2, None, False, f64=True) is True          # float32 does not depend on it
    for f64 in (False, True):
        assert lk.rows_route("cuda", torch.float16, 2, None, False, f64=f64) is False
        assert lk.rows_route("cuda", torch.bfloat16, 2, None, False, f64=f64) is False


@pytest.mark.parametrize("device,dtype,dim,hook,grad,enabled,want", ROUTES)
def test_every_fp32_refusal_still_refuses_with_the_keyword(device, dtype, dim, hook, grad, enabled, want):
    """The keyword widens the dtype test only: a row of the fp32 table that refuses for any other reason refuses with it, for a
    float32 and for a float64 right-hand side."""
    got = lk.rows_route(device, dtype, dim, hook, grad, enabled, f64=True)
    other = (device, dim, hook, grad, enabled) == ("cuda", 2, None, False, True)    # everything but the dtype allows it
    assert got is (other and dtype in (F32, F64))
    if dtype == F32:
        assert got is want
        assert lk.rows_route(device, F64, dim, hook, grad, enabled, f64=True) is want


def test_the_switch_exists_and_the_width_gate_is_single():
    assert isinstance(plx.RectangularLazyLattice.native_rows_f64, bool)
    assert plx.RectangularLazyLattice.native_min_columns == 101


def test_lattice_methods_exist():
    for name in ("rows_f64_kernels", "rows_kernels", "apply_rows", "splat_rows", "slice_rows"):
        assert callable(getattr(plx.Lattice, name)), name


def test_cpu_and_foreign_dtypes_are_refused_as_before():
    """A float64 CPU tensor is refused the way a float32 CPU tensor is (no CPU path), other dtypes stay a TypeError; both
    before the lattice is looked at."""
    lat = object.__new__(plx.Lattice)                      # never reached: the tensor checks come first
    for dtype in (F32, F64):
        t = torch.zeros(4, 2, dtype=dtype)
        with pytest.raises(ValueError, match="no CPU path"):
            plx.Lattice.apply_rows(lat, t, 0, 0, 4)
        with pytest.raises(ValueError, match="no CPU path"):
            plx.Lattice.splat_rows(lat, t, 0)
        with pytest.raises(ValueError, match="no CPU path"):
            plx.Lattice.slice_rows(lat, t, 0, 4)
    with pytest.raises(TypeError):
        plx.Lattice.apply_rows(lat, [[0.0]], 0, 0, 1)
