"""The rectangular product (plx_splat_rows / plx_slice_rows / plx_apply_rows) on the host: the C ABI's declarations and
exports, the argument checks that return before any launch, the routing predicate of RectangularLazyLattice, and the
padded path under the CPU hook, which the native route must leave exactly as it was."""
import ctypes
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice_kernel as lk
from oracle import oracle

def oracle_filter(src, ref, coeffs):
    out = oracle.filter(src.detach().numpy(), ref.detach().numpy(), coeffs.detach().numpy())
    return torch.from_numpy(out)


ROWS_SYMBOLS = ("plx_splat_rows", "plx_slice_rows", "plx_apply_rows", "plx_last_rows_kernels")


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_float * 1024)()                   # host memory: every call below returns before a launch could reach it
    p = ctypes.cast(buf, ctypes.c_void_p)
    p._keep = buf
    return p


@pytest.fixture()
def cpu_method():
    plx.LatticeFilterGeneral.method = staticmethod(oracle_filter)
    yield
    plx.LatticeFilterGeneral.method = None


def test_rows_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in ROWS_SYMBOLS:
        assert name in declared and name in _native._SIGNATURES, name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in ROWS_SYMBOLS:
        assert f" T {name}\n" in exported, name
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_rows_argument_checks_return_before_any_launch(lib, p):
    # a NULL lattice, and NULL buffers next to a lattice pointer that is never followed (the NULL test comes first)
    assert lib.plx_splat_rows(None, p, 0, 4, 1, p, None) == 1 and b"NULL" in lib.plx_last_error()
    assert lib.plx_slice_rows(None, p, 1, 0, 4, p, None) == 1 and b"NULL" in lib.plx_last_error()
    assert lib.plx_apply_rows(None, p, 0, 4, 1, p, 4, 4, None) == 1 and b"NULL" in lib.plx_last_error()
    assert lib.plx_splat_rows(p, None, 0, 4, 1, p, None) == 1 and b"plx_splat_rows" in lib.plx_last_error()
    assert lib.plx_splat_rows(p, p, 0, 4, 1, None, None) == 1
    assert lib.plx_slice_rows(p, None, 1, 0, 4, p, None) == 1 and b"plx_slice_rows" in lib.plx_last_error()
    assert lib.plx_slice_rows(p, p, 1, 0, 4, None, None) == 1
    assert lib.plx_apply_rows(p, None, 0, 4, 1, p, 4, 4, None) == 1 and b"plx_apply_rows" in lib.plx_last_error()
    assert lib.plx_apply_rows(p, p, 0, 4, 1, None, 4, 4, None) == 1
    buf = ctypes.create_string_buffer(64)
    assert lib.plx_last_rows_kernels(None, buf, 64) == 1
    assert lib.plx_last_rows_kernels(p, None, 64) == 1 and lib.plx_last_rows_kernels(p, buf, 0) == 1


F32, F64 = torch.float32, torch.float64
HOOK = staticmethod(oracle_filter)
ROUTES = [
    # device, dtype, dim, hook, positions want a gradient, switch -> native?
    ("cuda", F32, 2, None, False, True, True),
    ("cpu", F32, 2, None, False, True, False),
    ("cuda", F64, 2, None, False, True, False),
    ("cuda", torch.float16, 2, None, False, True, False),
    ("cuda", F32, 1, None, False, True, False),
    ("cuda", F32, 3, None, False, True, False),
    ("cuda", F32, 2, HOOK, False, True, False),
    ("cuda", F32, 2, None, True, True, False),
    ("cuda", F32, 2, None, False, False, False),
    ("cpu", F64, 3, HOOK, True, False, False),
]


@pytest.mark.parametrize("device,dtype,dim,hook,grad,enabled,want", ROUTES)
def test_routing_predicate(device, dtype, dim, hook, grad, enabled, want):
    assert lk.rows_route(device, dtype, dim, hook, grad, enabled) is want


def test_routing_default_is_on():
    assert plx.RectangularLazyLattice.native_rows is True
    assert lk.rows_route("cuda", F32, 2, None, False) is True


def test_routing_by_measured_width():
    """The shape gate: the native route from native_min_columns columns on (the width it was measured faster at)."""
    lo = plx.RectangularLazyLattice.native_min_columns
    assert lo == 101
    assert lk.rows_route("cuda", F32, 2, None, False, True, lo, lo) is True
    assert lk.rows_route("cuda", F32, 2, None, False, True, lo - 1, lo) is False
    assert lk.rows_route("cuda", F32, 2, None, False, True, 1, 1) is True
    assert lk.rows_route("cuda", F32, 2, None, False, False, 512, lo) is False


def test_padded_path_under_the_cpu_hook_is_untouched(cpu_method):
    g = torch.Generator().manual_seed(5)
    k = plx.RBFLattice(order=1, ard_num_dims=2)
    x, xs = torch.randn(60, 2, generator=g), torch.randn(17, 2, generator=g)
    V, G = torch.randn(60, 3, generator=g), torch.randn(17, 3, generator=g)
    outs = {}
    for on in (True, False):
        plx.RectangularLazyLattice.native_rows = on
        try:
            with torch.no_grad():
                R = k(xs, x)
                outs[on] = (R.matmul(V), R.t().matmul(G), R.t().t().matmul(V))
        finally:
            plx.RectangularLazyLattice.native_rows = True
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    assert outs[True][0].shape == (17, 3) and outs[True][1].shape == (60, 3)
    assert torch.equal(outs[True][0], outs[True][2])
    # ... and it is the padded product: one square filter over [x; xs] with zero rows for xs
    ell = k.lengthscale.detach()
    want = oracle_filter(torch.cat([V, torch.zeros(17, 3)]), torch.cat([x / ell, xs / ell]), k.dkernel_fn.get_coeffs())[60:]
    assert torch.equal(outs[True][0], want)


def test_lattice_methods_exist():
    for name in ("apply_rows", "splat_rows", "slice_rows", "rows_kernels", "accepts_rows"):
        assert callable(getattr(plx.Lattice, name)), name
    assert issubclass(lk.LatticeRowsProduct, torch.autograd.Function)
