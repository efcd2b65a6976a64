"""The float64 conjugate-gradient calls (plx_coldot_f64, plx_cg_step_update_f64, plx_cg_step_direction_f64,
plx_apply_affine_f64 and their two workspace sizes) on the host: the C ABI's declarations and exports, signatures that
mirror the fp32 calls, the workspace rule, the argument checks that return before any launch, and the dtype rule of
Lattice.apply_affine that needs no GPU (a mixed pair is a TypeError)."""
import ctypes
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native, solvers

CG64_SYMBOLS = ("plx_coldot_work_doubles", "plx_coldot_f64", "plx_cg_step_update_f64", "plx_cg_step_direction_f64",
                "plx_affine_dot_work_doubles", "plx_apply_affine_f64")
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


def test_cg64_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in CG64_SYMBOLS:
        assert name in declared and name in _native._SIGNATURES, name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in CG64_SYMBOLS:
        assert f" T {name}\n" in exported, name
    # the feature is detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_cg64_signatures_mirror_the_fp32_calls():
    sig = _native._SIGNATURES
    assert sig["plx_coldot_f64"] == sig["plx_coldot"]
    assert sig["plx_coldot_work_doubles"] == sig["plx_coldot_work_floats"]
    assert sig["plx_cg_step_update_f64"] == sig["plx_cg_step_update"]
    assert sig["plx_affine_dot_work_doubles"] == sig["plx_affine_dot_work_floats"]
    assert sig["plx_apply_affine_f64"] == sig["plx_apply_affine_dot"]
    # the direction step: the same arguments, the tolerance a double
    res32, args32 = sig["plx_cg_step_direction"]
    res64, args64 = sig["plx_cg_step_direction_f64"]
    assert res32 == res64 and len(args32) == len(args64)
    for a32, a64 in zip(args32, args64):
        assert a64 == (ctypes.c_double if a32 == ctypes.c_float else a32)


def test_coldot_work_doubles(lib):
    for vd in (-5, 0, 257, 1000):
        assert lib.plx_coldot_work_doubles(vd) == -1, vd
    sizes = [lib.plx_coldot_work_doubles(vd) for vd in range(1, 257)]
    assert all(s >= vd for vd, s in zip(range(1, 257), sizes))
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), "not monotone inside 1..256"
    # no lattice, no size
    assert lib.plx_affine_dot_work_doubles(None, 4) == -1


def _coldot(lib, p, **kw):
    a = dict(d_a=p, d_b=p, n=8, vd=4, d_out=p, d_work=p)
    a.update(kw)
    return lib.plx_coldot_f64(a["d_a"], a["d_b"], a["n"], a["vd"], a["d_out"], a["d_work"], None)


def _update(lib, p, n=8, vd=4, **kw):
    names = ("d_x", "d_r", "d_p", "d_ap", "d_rs", "d_pap", "d_active", "d_rs_new", "d_alpha", "d_work")
    a = {k: p for k in names}
    a.update(kw)
    return lib.plx_cg_step_update_f64(a["d_x"], a["d_r"], a["d_p"], a["d_ap"], a["d_rs"], a["d_pap"], a["d_active"], n, vd,
                                      a["d_rs_new"], a["d_alpha"], a["d_work"], None)


def _direction(lib, p, q, n=8, vd=4, **kw):
    names = ("d_p", "d_r", "d_rs_new", "d_rs", "d_active", "d_b_norm", "d_beta")
    a = {k: p for k in names}
    a["d_active_out"] = q
    a.update(kw)
    return lib.plx_cg_step_direction_f64(a["d_p"], a["d_r"], a["d_rs_new"], a["d_rs"], a["d_active"], a["d_b_norm"], 1e-8, n,
                                         vd, a["d_beta"], a["d_active_out"], None)


def test_cg64_argument_checks_return_before_any_launch(lib, p):
    """Every PLX_ERR_INVALID of the three vector calls, on host addresses: a launch that followed any of them would fault."""
    q = ctypes.c_void_p(p.value + 512 * 8)             # a second, distinct buffer (active_out != active)
    odd = ctypes.c_void_p(p.value + 4)                 # not 8-byte aligned
    # NULL pointers, one argument at a time
    for name in ("d_a", "d_b", "d_out", "d_work"):
        assert _coldot(lib, p, **{name: None}) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error(), name
    for name in ("d_x", "d_r", "d_p", "d_ap", "d_rs", "d_pap", "d_active", "d_rs_new", "d_alpha", "d_work"):
        assert _update(lib, p, **{name: None}) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error(), name
    for name in ("d_p", "d_r", "d_rs_new", "d_rs", "d_active", "d_b_norm", "d_beta", "d_active_out"):
        assert _direction(lib, p, q, **{name: None}) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error(), name
    # vd outside 1..256, n < 1
    for vd in (0, -1, 257):
        assert _coldot(lib, p, vd=vd) == PLX_ERR_INVALID and b"plx_coldot_f64" in lib.plx_last_error(), vd
        assert _update(lib, p, vd=vd) == PLX_ERR_INVALID and b"plx_cg_step_update_f64" in lib.plx_last_error(), vd
        assert _direction(lib, p, q, vd=vd) == PLX_ERR_INVALID and b"plx_cg_step_direction_f64" in lib.plx_last_error(), vd
    for n in (0, -7):
        assert _coldot(lib, p, n=n) == PLX_ERR_INVALID and b"positive" in lib.plx_last_error(), n
        assert _update(lib, p, n=n) == PLX_ERR_INVALID and b"positive" in lib.plx_last_error(), n
        assert _direction(lib, p, q, n=n) == PLX_ERR_INVALID and b"positive" in lib.plx_last_error(), n
    # a pointer that is not 8-byte aligned
    assert _coldot(lib, p, d_b=odd) == PLX_ERR_INVALID and b"8-byte" in lib.plx_last_error()
    assert _update(lib, p, d_ap=odd) == PLX_ERR_INVALID and b"8-byte" in lib.plx_last_error()
    assert _direction(lib, p, q, d_r=odd) == PLX_ERR_INVALID and b"8-byte" in lib.plx_last_error()
    # active_out aliasing active
    assert _direction(lib, p, p) == PLX_ERR_INVALID and b"different buffers" in lib.plx_last_error()
    # the affine product: a NULL lattice, and NULL buffers next to a lattice pointer that is never followed
    assert lib.plx_apply_affine_f64(None, p, 1, q, p, None, None, None) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error()
    assert lib.plx_apply_affine_f64(p, None, 1, q, p, None, None, None) == PLX_ERR_INVALID
    assert b"plx_apply_affine_f64" in lib.plx_last_error()
    assert lib.plx_apply_affine_f64(p, p, 1, None, p, None, None, None) == PLX_ERR_INVALID


def test_apply_affine_mixed_dtypes_are_a_type_error():
    """A float64 matrix next to a float32 (a, b), or the reverse, is refused by its dtypes before anything else is looked
    at -- wherever the tensors live, so no lattice has to be built for it."""
    lat = object.__new__(plx.Lattice)                  # no handle: the dtype rule comes before any use of it
    v64, v32 = torch.randn(6, 2, dtype=torch.float64), torch.randn(6, 2)
    ss64, ss32 = torch.ones(2, dtype=torch.float64), torch.ones(2)
    for v, ss in ((v64, ss32), (v32, ss64)):
        for want_dot in (False, True):
            with pytest.raises(TypeError, match="both"):
                lat.apply_affine(v, ss, want_dot=want_dot)


def test_solver_switch_and_dtype_rule():
    assert solvers.NATIVE_CG_F64 is True
    a32, a64 = torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.float64)
    # CPU tensors never go native, in either precision; the rule itself is about one dtype for all
    assert not solvers._native_ok(a32) and not solvers._native_ok(a64, f64_ok=True)
    assert solvers._f64_native(a64) and not solvers._f64_native(a32)
    solvers.NATIVE_CG_F64 = False
    try:
        assert not solvers._f64_native(a64)
    finally:
        solvers.NATIVE_CG_F64 = True
    # the torch loop still solves a double system on the CPU
    A = torch.eye(4, dtype=torch.float64) * 2.0
    X, info = solvers.batched_cg(lambda V: A @ V, torch.ones(4, 2, dtype=torch.float64), tol=1e-12)
    assert X.dtype == torch.float64 and torch.allclose(X, torch.full_like(X, 0.5))
