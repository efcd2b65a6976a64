"""The one-sided float64 position gradient of the rectangular product (plx_backward_splat_rows_f64,
plx_backward_contract_rows_f64, plx_apply_backward_rows_f64) on the host: the C ABI's declarations and exports, the argument
checks that need no built lattice and return before any launch, the shape predicate at its edges, the dtype rule of
Lattice.apply_backward_rows, the switch and the routing predicate's grad_f64 keyword, and the split of the padded gradient
into two one-sided ones, on the CPU with Lattice64."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice_kernel as lk
from tests.lattice64 import Lattice64, cloud
from tests.rows_backward64 import U, depth64, one_sided, scatter_sides
from tests.test_backward_f64_gpu import dkernel, ratio_to_bar, reference
from tests.test_rows_host import ROUTES

SYMBOLS = ("plx_backward_splat_rows_f64", "plx_backward_contract_rows_f64", "plx_apply_backward_rows_f64")
PLX_ERR_INVALID = 1
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def bufs():
    """Six distinct 16-byte aligned host addresses: every call below returns before a launch could reach them, and before
    the lattice pointer (one of them) is followed."""
    raw = (ctypes.c_double * 1026)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    out = [ctypes.c_void_p(base + i * 128 * 8) for i in range(6)]
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
    assert sig["plx_backward_splat_rows_f64"] == (i32, [vp, vp, i64, i64, vp, i32, vp, vp])
    # (lat, values, b, b_begin, b_count, x, nrhs, grad_x, filtered, stream)
    assert sig["plx_backward_contract_rows_f64"] == (i32, [vp, vp, vp, i64, i64, vp, i32, vp, vp, vp])
    # (lat, a, a_begin, a_count, b, b_begin, b_count, x, nrhs, grad_x, filtered, stream)
    assert sig["plx_apply_backward_rows_f64"] == (i32, [vp, vp, i64, i64, vp, i64, i64, vp, i32, vp, vp, vp])


def _splat(lib, lat, a, x, values, nrhs=2, count=4):
    return lib.plx_backward_splat_rows_f64(lat, a, 0, count, x, nrhs, values, None)


def _contract(lib, lat, values, b, x, gx, fl, nrhs=2, count=4):
    return lib.plx_backward_contract_rows_f64(lat, values, b, 0, count, x, nrhs, gx, fl, None)


def _apply(lib, lat, a, b, x, gx, fl, nrhs=2, a_count=4, b_count=4):
    return lib.plx_apply_backward_rows_f64(lat, a, 0, a_count, b, 4, b_count, x, nrhs, gx, fl, None)


def test_argument_checks_return_before_any_launch(lib, bufs):
    """Every PLX_ERR_INVALID that needs no built lattice, on host addresses: the lattice pointer is never followed and a
    launch that followed any of these would fault."""
    lat, a, b, x, o1, o2 = bufs
    odd = lambda p: ctypes.c_void_p(p.value + 4)             # noqa: E731  off 8-byte alignment
    err = lib.plx_last_error
    # a NULL lattice
    assert _splat(lib, None, a, x, o1) == PLX_ERR_INVALID and b"NULL" in err()
    assert _contract(lib, None, o1, b, x, o2, None) == PLX_ERR_INVALID and b"NULL" in err()
    assert _apply(lib, None, a, b, x, o1, o2) == PLX_ERR_INVALID and b"NULL" in err()
    # NULL buffers, one at a time; d_filtered alone may be NULL, so that call gets past the NULL test to the next refusal
    for i in range(3):
        args = [a, x, o1]
        args[i] = None
        assert _splat(lib, lat, *args) == PLX_ERR_INVALID and b"plx_backward_splat_rows_f64: NULL" in err(), i
    for i in range(4):
        args = [o1, b, x, o2]
        args[i] = None
        assert _contract(lib, lat, *args, None) == PLX_ERR_INVALID and b"plx_backward_contract_rows_f64: NULL" in err(), i
    for i in range(4):
        args = [a, b, x, o1]
        args[i] = None
        assert _apply(lib, lat, *args, None) == PLX_ERR_INVALID and b"plx_apply_backward_rows_f64: NULL" in err(), i
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
    # a pointer off 8-byte alignment, every argument in turn
    for i in range(3):
        args = [a, x, o1]
        args[i] = odd(args[i])
        assert _splat(lib, lat, *args) == PLX_ERR_INVALID and b"8-byte" in err(), i
    for i in range(5):
        args = [o1, b, x, o2, bufs[0]]
        args[i] = odd(args[i])
        assert _contract(lib, lat, *args) == PLX_ERR_INVALID and b"8-byte" in err(), i
    for i in range(5):
        args = [a, b, x, o1, o2]
        args[i] = odd(args[i])
        assert _apply(lib, lat, *args) == PLX_ERR_INVALID and b"8-byte" in err(), i
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
    # tests/test_rows_backward_f64_gpu.py)


def test_backward_rows_f64_ok_at_its_edges():
    ok = plx.Lattice.backward_rows_f64_ok
    assert plx.Lattice.BACKWARD_ROWS_F64_MAX_STRIDE == 2048
    assert ok(1, 1) is True                            # H = 2, the smallest row
    assert ok(256, 7) is True                          # stride exactly 2048
    assert ok(257, 7) is False                         # 2056
    # H = 2046 is within the limit whatever (nrhs, d) make it; the next row of d = 21 (H = 2068) is not
    assert ok(93, 21) is True and ok(1023, 1) is True
    assert ok(94, 21) is False
    assert ok(2047, 0) is False                        # d < 1, whatever the width
    assert ok(89, 22) is True                          # H = 2047 rounds up to 2048
    assert ok(1024, 1) is True and ok(1025, 1) is False
    assert not ok(0, 8) and not ok(-1, 8) and not ok(8, 0)
    # the square predicate is where it was
    assert plx.Lattice.backward_f64_ok(128, 7) and not plx.Lattice.backward_f64_ok(129, 7)


def test_apply_backward_rows_has_no_fp32_form():
    """Any float32 tensor among the three is refused by the dtypes before anything else is looked at -- wherever the tensors
    live, so no lattice has to be built for it."""
    lat = object.__new__(plx.Lattice)                  # no handle: the dtype rule comes before any use of it
    t64 = lambda *s: torch.randn(*s, dtype=F64)        # noqa: E731
    t32 = lambda *s: torch.randn(*s)                   # noqa: E731
    for mask in range(0, 7):                           # every combination but all-fp64; 0 is all-fp32
        a, b, x = ((t64 if mask >> i & 1 else t32)(6, k) for i, k in enumerate((2, 2, 3)))
        for want in (True, False):
            with pytest.raises(TypeError, match="no fp32 form"):
                lat.apply_backward_rows(a, 0, b, 0, x, want_filtered=want)
    with pytest.raises(TypeError):
        lat.apply_backward_rows([[0.0]], 0, t64(1, 1), 0, t64(1, 1))
    with pytest.raises(ValueError, match="no CPU path"):
        lat.apply_backward_rows(t64(6, 2), 0, t64(6, 2), 0, t64(6, 3))


def test_the_switch_exists_and_is_off():
    assert plx.RectangularLazyLattice.native_rows_grad_f64 is False
    assert plx.RectangularLazyLattice.native_rows_f64 is False and plx.RectangularLazyLattice.native_min_columns == 101
    assert callable(plx.Lattice.apply_backward_rows)


@pytest.mark.parametrize("device,dtype,dim,hook,grad,enabled,want", ROUTES)
def test_routing_predicate_without_the_keyword_is_unchanged(device, dtype, dim, hook, grad, enabled, want):
    assert lk.rows_route(device, dtype, dim, hook, grad, enabled) is want
    assert lk.rows_route(device, dtype, dim, hook, grad, enabled, grad_f64=False) is want
    for f64 in (False, True):
        assert lk.rows_route(device, dtype, dim, hook, grad, enabled, f64=f64) is \
            lk.rows_route(device, dtype, dim, hook, grad, enabled, f64=f64, grad_f64=False)
    # with it: only a CUDA float64 2-D right-hand side whose positions want a gradient, no hook, the route switched on
    got = lk.rows_route(device, dtype, dim, hook, grad, enabled, grad_f64=True)
    assert got is False if dtype != F64 else got is ((device, dim, hook, grad, enabled) == ("cuda", 2, None, True, True))
    got64 = lk.rows_route(device, F64, dim, hook, grad, enabled, grad_f64=True)
    assert got64 is ((device, dim, hook, grad, enabled) == ("cuda", 2, None, True, True))


def test_routing_predicate_with_the_grad_keyword():
    assert lk.rows_route("cuda", F64, 2, None, True, grad_f64=True) is True
    assert lk.rows_route("cuda", F64, 2, None, True, True, 1, 101, grad_f64=True) is True     # no width gate
    assert lk.rows_route("cuda", F64, 2, None, False, grad_f64=True) is False                 # nothing wants a gradient
    assert lk.rows_route("cuda", F32, 2, None, True, grad_f64=True) is False                  # no fp32 form
    assert lk.rows_route("cuda", F32, 2, None, True, f64=True, grad_f64=True) is False
    assert lk.rows_route("cpu", F64, 2, None, True, grad_f64=True) is False
    assert lk.rows_route("cuda", F64, 3, None, True, grad_f64=True) is False
    assert lk.rows_route("cuda", F64, 2, object(), True, grad_f64=True) is False
    assert lk.rows_route("cuda", F64, 2, None, True, False, grad_f64=True) is False
    # without it a wanted gradient refuses, as before
    assert lk.rows_route("cuda", F64, 2, None, True, f64=True) is False
    assert lk.rows_route("cuda", F32, 2, None, True) is False


SPLITS = [((0, 200), (200, 101), True), ((0, 180), (120, 181), False), ((75, 150), (75, 150), False)]


@pytest.fixture(scope="module")
def split_problem():
    n, d, L = 301, 3, 2
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    x = cloud("gauss1", n, d, seed=4, coeffs=dtaps).astype(np.float64)
    x *= 1.0 + 1e-9 * np.random.default_rng(5).standard_normal(x.shape)
    return n, d, L, x, Lattice64(x, dtaps)


@pytest.mark.parametrize("src_range,out_range,disjoint", SPLITS)
def test_the_split_on_the_cpu(split_problem, src_range, out_range, disjoint):
    """G lives on the out rows, S on the source rows: the padded gradient (tests/test_backward_f64_gpu.reference) against the
    two one-sided references added into [n, d].  Disjoint ranges: identical.  Overlapping or equal ranges: within the padded
    bar 2 (k + 4 (L + 1)) U T'.  The filtered columns equal the padded wg rows in every case."""
    n, d, L, x, l64 = split_problem
    rng = np.random.default_rng(n + src_range[1])
    (sb, sc), (ob, oc) = src_range, out_range
    g, s = rng.standard_normal((oc, L)), rng.standard_normal((sc, L))
    G, S = np.zeros((n, L)), np.zeros((n, L))
    G[ob:ob + oc], S[sb:sb + sc] = g, s
    want, want_gs, T, _ = reference(G, S, x, l64)
    on_src, filt, T_src, _ = one_sided(g, out_range, s, src_range, x, l64)          # the source rows' positions, and wg there
    on_out, _, T_out, _ = one_sided(s, src_range, g, out_range, x, l64)             # the out rows' positions
    got = scatter_sides(n, d, src_range, out_range, on_src, on_out)
    assert np.array_equal(filt, want_gs[sb:sb + sc])
    if disjoint:
        assert np.array_equal(got, want)
        assert np.array_equal(scatter_sides(n, d, src_range, out_range, T_src, T_out), T)
    else:
        k = depth64(l64)
        r = ratio_to_bar(got.astype(np.float64), want, T, 2 * (k + 4 * (L + 1)) * U, "split")
        assert r <= 1.0, r
    # rows outside both ranges carry nothing
    outside = np.ones(n, bool)
    outside[sb:sb + sc] = False
    outside[ob:ob + oc] = False
    assert not got[outside].any() and not want[outside].any()
