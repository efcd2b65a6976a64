"""The float64 product (plx_splat_f64 / plx_blur_f64 / plx_slice_f64 / plx_apply_f64) on the host: the C ABI's declarations
and exports, the argument checks that return before any launch, the value-row stride in doubles, and the dtype rules of the
Python boundary that need no GPU (a mixed pair is a TypeError, a CPU tensor has no path in either precision)."""
import ctypes
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice_kernel as lk

F64_SYMBOLS = ("plx_values_stride_f64", "plx_splat_f64", "plx_blur_f64", "plx_slice_f64", "plx_apply_f64",
               "plx_last_f64_kernels")
PLX_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_double * 1024)()                  # host memory: every call below returns before a launch could reach it
    p = ctypes.cast(buf, ctypes.c_void_p)
    p._keep = buf
    return p


def test_f64_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in F64_SYMBOLS:
        assert name in declared and name in _native._SIGNATURES, name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in F64_SYMBOLS:
        assert f" T {name}\n" in exported, name
    # the feature is detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_f64_signatures_mirror_the_fp32_stages():
    for name in ("plx_splat", "plx_blur", "plx_slice", "plx_apply"):
        assert _native._SIGNATURES[name + "_f64"] == _native._SIGNATURES[name], name
    assert _native._SIGNATURES["plx_last_f64_kernels"] == _native._SIGNATURES["plx_last_rows_kernels"]


def test_values_stride_f64(lib):
    want = {1: 1, 2: 2, 3: 4, 4: 4, 5: 6, 11: 12, 12: 12, 101: 102, 520: 520, 521: 522}
    for vd, stride in want.items():
        assert lib.plx_values_stride_f64(vd) == stride, vd
        assert plx.Lattice.values_stride(vd, torch.float64) == stride
    assert lib.plx_values_stride_f64(0) == -1 and lib.plx_values_stride_f64(-3) == -1
    # rows are whole 16-byte vectors in both precisions
    for vd in range(2, 70):
        assert lib.plx_values_stride_f64(vd) * 8 % 16 == 0 and lib.plx_values_stride_f64(vd) >= vd
        assert plx.Lattice.values_stride(vd) == lib.plx_values_stride(vd)


def test_f64_argument_checks_return_before_any_launch(lib, p):
    flag = ctypes.c_int(0)
    # a NULL lattice, and NULL buffers next to a lattice pointer that is never followed (the NULL test comes first)
    assert lib.plx_splat_f64(None, p, 1, p, None) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error()
    assert lib.plx_blur_f64(None, p, p, 1, ctypes.byref(flag), None) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error()
    assert lib.plx_slice_f64(None, p, 1, p, None) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error()
    assert lib.plx_apply_f64(None, p, 1, p, None) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error()
    assert lib.plx_splat_f64(p, None, 1, p, None) == PLX_ERR_INVALID and b"plx_splat_f64" in lib.plx_last_error()
    assert lib.plx_splat_f64(p, p, 1, None, None) == PLX_ERR_INVALID
    assert lib.plx_blur_f64(p, None, p, 1, ctypes.byref(flag), None) == PLX_ERR_INVALID and b"plx_blur_f64" in lib.plx_last_error()
    assert lib.plx_blur_f64(p, p, None, 1, ctypes.byref(flag), None) == PLX_ERR_INVALID
    assert lib.plx_slice_f64(p, None, 1, p, None) == PLX_ERR_INVALID and b"plx_slice_f64" in lib.plx_last_error()
    assert lib.plx_slice_f64(p, p, 1, None, None) == PLX_ERR_INVALID
    assert lib.plx_apply_f64(p, None, 1, p, None) == PLX_ERR_INVALID and b"plx_apply_f64" in lib.plx_last_error()
    assert lib.plx_apply_f64(p, p, 1, None, None) == PLX_ERR_INVALID
    buf = ctypes.create_string_buffer(64)
    assert lib.plx_last_f64_kernels(None, buf, 64) == PLX_ERR_INVALID
    assert lib.plx_last_f64_kernels(p, None, 64) == PLX_ERR_INVALID and lib.plx_last_f64_kernels(p, buf, 0) == PLX_ERR_INVALID


def test_mixed_dtypes_stay_a_type_error():
    """One float64 tensor next to a float32 one is refused by its dtypes, wherever the tensors live."""
    src64, ref32 = torch.randn(6, 2, dtype=torch.float64), torch.randn(6, 3)
    taps = torch.tensor([0.5, 1.0, 0.5])
    for a, b in ((src64, ref32), (src64.float(), ref32.double())):
        with pytest.raises(TypeError):
            plx.filter(a, b, taps)
        with pytest.raises(TypeError):
            lk.cached_filter(a, b, taps)


def test_float64_cpu_tensors_have_no_path():
    plx.LatticeFilterGeneral.method = None
    dk = plx.DiscretizedKernelFN(plx.rbf, 1)
    x = torch.randn(8, 2, dtype=torch.float64)
    v = torch.randn(8, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU path"):
        plx.LatticeFilterGeneral.apply(v, x, dk)
    with pytest.raises(ValueError, match="no CPU path"):
        plx.filter(v, x, torch.tensor([0.5, 1.0, 0.5]))


def test_rows_route_stays_fp32():
    assert lk.rows_route("cuda", torch.float64, 2, None, False) is False


def test_lattice_methods_exist():
    import inspect
    assert callable(plx.Lattice.f64_kernels)
    for name in ("values_stride", "new_values"):
        assert "dtype" in inspect.signature(getattr(plx.Lattice, name)).parameters, name
