"""The float64 position gradient (plx_backward_splat_f64, plx_backward_contract_f64, plx_apply_backward_f64) on the host: the
C ABI's declarations and exports, a signature that mirrors plx_apply_backward, the argument checks that need no built
lattice and return before any launch, the dtype rule of Lattice.apply_backward (a mixed combination is a TypeError) and the
column limit Lattice.backward_f64_ok names."""
import ctypes
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native

BACKWARD64_SYMBOLS = ("plx_backward_splat_f64", "plx_backward_contract_f64", "plx_apply_backward_f64")
PLX_ERR_INVALID = 1


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


def test_backward64_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in BACKWARD64_SYMBOLS:
        assert name in declared and name in _native._SIGNATURES, name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in BACKWARD64_SYMBOLS:
        assert f" T {name}\n" in exported, name
    # the feature is detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_backward64_signature_mirrors_the_fp32_call():
    sig = _native._SIGNATURES
    assert sig["plx_apply_backward_f64"] == sig["plx_apply_backward"]
    res, args = sig["plx_apply_backward_f64"]
    # the staged calls: the same arguments with d_values in place of the outputs (splat) or in front (contract)
    assert sig["plx_backward_splat_f64"] == (res, args[:5] + [args[5], args[7]])
    assert sig["plx_backward_contract_f64"] == (res, [args[0], ctypes.c_void_p] + args[1:])


def _splat(lib, lat, g, s, x, values, nrhs=2):
    return lib.plx_backward_splat_f64(lat, g, s, x, nrhs, values, None)


def _contract(lib, lat, values, g, s, x, gx, gs, nrhs=2):
    return lib.plx_backward_contract_f64(lat, values, g, s, x, nrhs, gx, gs, None)


def _apply(lib, lat, g, s, x, gx, gs, nrhs=2):
    return lib.plx_apply_backward_f64(lat, g, s, x, nrhs, gx, gs, None)


def test_backward64_argument_checks_return_before_any_launch(lib, bufs):
    """Every PLX_ERR_INVALID that needs no built lattice, on host addresses: the lattice pointer is never followed and a
    launch that followed any of these would fault."""
    lat, g, s, x, a, b = bufs
    odd = lambda p: ctypes.c_void_p(p.value + 4)             # noqa: E731  off 8-byte alignment
    half = lambda p: ctypes.c_void_p(p.value + 8)            # noqa: E731  8-byte but not 16-byte aligned
    err = lib.plx_last_error
    # a NULL lattice
    assert _splat(lib, None, g, s, x, a) == PLX_ERR_INVALID and b"NULL" in err()
    assert _contract(lib, None, a, g, s, x, b, None) == PLX_ERR_INVALID and b"NULL" in err()
    assert _apply(lib, None, g, s, x, a, b) == PLX_ERR_INVALID and b"NULL" in err()
    # NULL buffers, one at a time; d_grad_src alone may be NULL, so that call gets past the NULL test to the next refusal
    for i in range(4):
        args = [g, s, x, a]
        args[i] = None
        assert _splat(lib, lat, *args) == PLX_ERR_INVALID and b"plx_backward_splat_f64: NULL" in err(), i
    for i in range(5):
        args = [a, g, s, x, b]
        args[i] = None
        assert _contract(lib, lat, *args, None) == PLX_ERR_INVALID and b"plx_backward_contract_f64: NULL" in err(), i
    for i in range(4):
        args = [g, s, x, a]
        args[i] = None
        assert _apply(lib, lat, *args, None) == PLX_ERR_INVALID and b"plx_apply_backward_f64: NULL" in err(), i
    assert _apply(lib, lat, g, s, x, a, None, nrhs=0) == PLX_ERR_INVALID and b"positive" in err()
    # nrhs < 1
    for nrhs in (0, -3):
        assert _splat(lib, lat, g, s, x, a, nrhs=nrhs) == PLX_ERR_INVALID and b"positive" in err()
        assert _contract(lib, lat, a, g, s, x, b, None, nrhs=nrhs) == PLX_ERR_INVALID and b"positive" in err()
        assert _apply(lib, lat, g, s, x, a, b, nrhs=nrhs) == PLX_ERR_INVALID and b"positive" in err()
    # a pointer off 8-byte alignment, every argument in turn
    for i in range(4):
        args = [g, s, x, a]
        args[i] = odd(args[i])
        assert _splat(lib, lat, *args) == PLX_ERR_INVALID and b"8-byte" in err(), i
    for i in range(6):
        args = [a, g, s, x, b, bufs[0]]
        args[i] = odd(args[i])
        assert _contract(lib, lat, *args) == PLX_ERR_INVALID and b"8-byte" in err(), i
    for i in range(5):
        args = [g, s, x, a, b]
        args[i] = odd(args[i])
        assert _apply(lib, lat, *args) == PLX_ERR_INVALID and b"8-byte" in err(), i
    # outputs aliasing inputs or each other
    for inp in (g, s, x):
        assert _splat(lib, lat, g, s, x, inp) == PLX_ERR_INVALID and b"alias" in err()
        assert _apply(lib, lat, g, s, x, inp, None) == PLX_ERR_INVALID and b"alias" in err()
        assert _apply(lib, lat, g, s, x, a, inp) == PLX_ERR_INVALID and b"alias" in err()
    for inp in (a, g, s, x):
        assert _contract(lib, lat, a, g, s, x, inp, None) == PLX_ERR_INVALID and b"alias" in err()
        assert _contract(lib, lat, a, g, s, x, b, inp) == PLX_ERR_INVALID and b"alias" in err()
    assert _apply(lib, lat, g, s, x, a, a) == PLX_ERR_INVALID and b"alias" in err()
    assert _contract(lib, lat, a, g, s, x, b, b) == PLX_ERR_INVALID and b"alias" in err()
    # (d_values off 16-byte alignment needs a built lattice to get that far: tests/test_backward_f64_gpu.py)
    assert half(a).value % 16 == 8


def test_apply_backward_mixed_dtypes_are_a_type_error():
    """One float64 tensor next to a float32 one is refused by the dtypes before anything else is looked at -- wherever the
    tensors live, so no lattice has to be built for it."""
    lat = object.__new__(plx.Lattice)                  # no handle: the dtype rule comes before any use of it
    t64 = lambda *s: torch.randn(*s, dtype=torch.float64)     # noqa: E731
    t32 = lambda *s: torch.randn(*s)                          # noqa: E731
    for mask in range(1, 7):                                  # every combination but all-fp32 and all-fp64
        g, s, x = ((t64 if mask >> i & 1 else t32)(6, k) for i, k in enumerate((2, 2, 3)))
        for want in (True, False):
            with pytest.raises(TypeError, match="all be float32 or all float64"):
                lat.apply_backward(g, s, x, want_grad_src=want)


def test_backward_f64_ok_at_its_edges():
    ok = plx.Lattice.backward_f64_ok
    assert plx.Lattice.BACKWARD_F64_MAX_COLUMNS == 2048
    assert ok(1, 1)                                    # 4 columns: the smallest row
    assert ok(11, 8) and ok(20, 25)                    # the training shape; 1040 columns
    assert ok(32, 31) and ok(1024, 0) is False         # exactly 2048 columns; d < 1
    assert not ok(41, 24)                              # 2050 columns
    assert not ok(33, 31) and not ok(0, 8) and not ok(-1, 8)
    assert ok(128, 7) and not ok(129, 7)               # 2048 / 2064
    # the fp32 predicate is where it was
    assert plx.Lattice.backward_fusable(11, 8) and not plx.Lattice.backward_fusable(1, 1)


def test_switch_exists_and_is_a_bool():
    assert isinstance(plx.LatticeFilterGeneral.fused_backward_f64, bool)
    assert plx.LatticeFilterGeneral.fused_backward is True
