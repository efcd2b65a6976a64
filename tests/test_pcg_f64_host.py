"""The float64 preconditioner calls (plx_pcg_gram_f64, plx_pcg_project_f64, plx_pcg_apply_f64, plx_pcg_step_direction_f64,
plx_pcg_work_doubles) on the host: declarations, exports and signatures, the workspace rule, every argument check that
returns before any launch, the solver switch, and the route a CPU double model keeps."""
import ctypes
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native, solvers

PCG64_SYMBOLS = ("plx_pcg_work_doubles", "plx_pcg_gram_f64", "plx_pcg_project_f64", "plx_pcg_apply_f64",
                 "plx_pcg_step_direction_f64")
PLX_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_double * 1024)()                  # host memory: every call below returns before a launch could reach it
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 63) // 64 * 64)        # 64-byte aligned, 900 doubles of room behind it
    p._keep = buf
    return p


def test_pcg64_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in PCG64_SYMBOLS:
        assert name in declared and name in _native._SIGNATURES and name in _native.OPTIONAL_SYMBOLS, name
        assert hasattr(lib, name), name
    assert _native.has_symbols(*PCG64_SYMBOLS) and not _native.has_symbols("plx_no_such_call")
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in PCG64_SYMBOLS:
        assert f" T {name}\n" in exported, name
    # the feature is detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_pcg64_signatures():
    """The fp32 calls' arguments without factor_type; the tolerance a double."""
    sig = _native._SIGNATURES
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert sig["plx_pcg_work_doubles"] == sig["plx_pcg_work_floats"]
    res, args = sig["plx_pcg_project"]
    assert sig["plx_pcg_project_f64"] == (res, args[:1] + args[2:])
    res, args = sig["plx_pcg_apply"]
    assert sig["plx_pcg_apply_f64"] == (res, args[:1] + args[2:])
    assert sig["plx_pcg_gram_f64"] == (i32, [vp, i64, i32, vp, i64, i32, vp, vp, vp])
    res32, args32 = sig["plx_pcg_step_direction"]
    res64, args64 = sig["plx_pcg_step_direction_f64"]
    assert res32 == res64 and len(args32) == len(args64)
    for a32, a64 in zip(args32, args64):
        assert a64 == (ctypes.c_double if a32 == ctypes.c_float else a32)


def test_pcg_work_doubles(lib):
    for n, kp, t in ((0, 16, 1), (-3, 16, 1), (64, 0, 1), (64, 8, 1), (64, 24, 1), (64, 1040, 1), (64, 16, 0), (64, 16, 17),
                     (64, 16, -1)):
        assert lib.plx_pcg_work_doubles(n, kp, t) == -1, (n, kp, t)
    ns = (1, 63, 64, 65, 255, 256, 257, 1023, 3077, 10 ** 6, 10 ** 7)
    for t in (1, 11, 16):
        for kp in (16, 32, 112, 1024):
            sizes = [lib.plx_pcg_work_doubles(n, kp, t) for n in ns]
            assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])), (kp, t, sizes)
    for n in (1, 3077):
        for t in (1, 16):
            sizes = [lib.plx_pcg_work_doubles(n, kp, t) for kp in range(16, 1025, 16)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n, t)
        for kp in (16, 112):
            sizes = [lib.plx_pcg_work_doubles(n, kp, t) for t in range(1, 17)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n, kp)
    # room for one partial row of t doubles per 256 rows behind the gram partials
    assert lib.plx_pcg_work_doubles(3077, 112, 11) - lib.plx_pcg_work_doubles(1, 112, 11) >= (3077 // 256) * 11


def _gram(lib, p, **kw):
    a = dict(d_lt=p, ld=64, kp=16, d_r=p, n=8, t=4, d_g=p, d_work=p)
    a.update(kw)
    return lib.plx_pcg_gram_f64(a["d_lt"], a["ld"], a["kp"], a["d_r"], a["n"], a["t"], a["d_g"], a["d_work"], None)


def _project(lib, p, **kw):
    a = dict(d_lt=p, ld=64, kp=16, d_r=p, n=8, t=4, d_cinv=p, d_t=p, d_work=p)
    a.update(kw)
    return lib.plx_pcg_project_f64(a["d_lt"], a["ld"], a["kp"], a["d_r"], a["n"], a["t"], a["d_cinv"], a["d_t"], a["d_work"], None)


def _apply(lib, p, q, **kw):
    a = dict(d_lt=p, ld=64, kp=16, k=16, d_r=p, n=8, t=4, d_t=p, d_scale=p, d_z=q, d_rz=p, d_work=p)
    a.update(kw)
    return lib.plx_pcg_apply_f64(a["d_lt"], a["ld"], a["kp"], a["k"], a["d_r"], a["n"], a["t"], a["d_t"], a["d_scale"], a["d_z"],
                                 a["d_rz"], a["d_work"], None)


def _direction(lib, p, q, n=8, vd=4, **kw):
    names = ("d_p", "d_z", "d_rz_new", "d_rz", "d_rr", "d_active", "d_b_norm", "d_beta")
    a = {k: p for k in names}
    a["d_active_out"] = q
    a.update(kw)
    return lib.plx_pcg_step_direction_f64(a["d_p"], a["d_z"], a["d_rz_new"], a["d_rz"], a["d_rr"], a["d_active"], a["d_b_norm"],
                                          1e-8, n, vd, a["d_beta"], a["d_active_out"], None)


def test_pcg64_argument_checks_return_before_any_launch(lib, p):
    """Every PLX_ERR_INVALID of the four calls, on host addresses: a launch that followed any of them would fault."""
    q = ctypes.c_void_p(p.value + 512 * 8)             # a second, distinct buffer (Z != R, active_out != active)
    odd = ctypes.c_void_p(p.value + 4)                 # not 8-byte aligned
    off8 = ctypes.c_void_p(p.value + 8)                # 8-byte but not 16-byte aligned: refused for the factor only
    calls = {"plx_pcg_gram_f64": lambda **kw: _gram(lib, p, **kw), "plx_pcg_project_f64": lambda **kw: _project(lib, p, **kw),
             "plx_pcg_apply_f64": lambda **kw: _apply(lib, p, q, **kw)}
    pointers = {"plx_pcg_gram_f64": ("d_lt", "d_r", "d_g", "d_work"),
                "plx_pcg_project_f64": ("d_lt", "d_r", "d_cinv", "d_t", "d_work"),
                "plx_pcg_apply_f64": ("d_lt", "d_r", "d_t", "d_scale", "d_z", "d_work")}
    for who, call in calls.items():
        for name in pointers[who]:
            assert call(**{name: None}) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error(), (who, name)
            if name != "d_lt":
                assert call(**{name: odd}) == PLX_ERR_INVALID and b"8-byte" in lib.plx_last_error(), (who, name)
        for t in (0, -1, 17):
            assert call(t=t) == PLX_ERR_INVALID and who.encode() in lib.plx_last_error(), (who, t)
        for n in (0, -7):
            assert call(n=n) == PLX_ERR_INVALID and who.encode() in lib.plx_last_error(), (who, n)
        # the factor's shape contract: ld < n, ld no multiple of 64, kp no multiple of 16 / below 16 / above 1024, alignment
        for bad in (dict(ld=64, n=65), dict(ld=96, n=8), dict(ld=0, n=8), dict(kp=0), dict(kp=8), dict(kp=24), dict(kp=1040)):
            assert call(**bad) == PLX_ERR_INVALID and who.encode() in lib.plx_last_error(), (who, bad)
        for ptr in (off8, odd):
            assert call(d_lt=ptr) == PLX_ERR_INVALID and b"16-byte" in lib.plx_last_error(), who
    # apply: k outside 0..kp, Z aliasing R, a misaligned rz (NULL is allowed: it is optional)
    for k in (17, 1000, -1):
        assert _apply(lib, p, q, k=k) == PLX_ERR_INVALID and b"k = " in lib.plx_last_error(), k
    assert _apply(lib, p, p) == PLX_ERR_INVALID and b"different buffers" in lib.plx_last_error()
    assert _apply(lib, p, q, d_rz=odd) == PLX_ERR_INVALID and b"8-byte" in lib.plx_last_error()
    # direction
    for name in ("d_p", "d_z", "d_rz_new", "d_rz", "d_rr", "d_active", "d_b_norm", "d_beta", "d_active_out"):
        assert _direction(lib, p, q, **{name: None}) == PLX_ERR_INVALID and b"NULL" in lib.plx_last_error(), name
        assert _direction(lib, p, q, **{name: odd}) == PLX_ERR_INVALID and b"8-byte" in lib.plx_last_error(), name
    for vd in (0, -1, 257):
        assert _direction(lib, p, q, vd=vd) == PLX_ERR_INVALID and b"plx_pcg_step_direction_f64" in lib.plx_last_error(), vd
    for n in (0, -7):
        assert _direction(lib, p, q, n=n) == PLX_ERR_INVALID and b"positive" in lib.plx_last_error(), n
    assert _direction(lib, p, p) == PLX_ERR_INVALID and b"different buffers" in lib.plx_last_error()


def test_switch_and_cpu_route(monkeypatch):
    assert solvers.NATIVE_PCG_F64 is True
    assert issubclass(solvers.LatticePreconditioner64, solvers.LatticePreconditioner)
    # a CPU double x keeps the torch form (recorded here instead of built: the product itself has no CPU path)
    built = []

    class Recorded:
        def __init__(self, kmatmul, n, outputscale, noise, rank, device, dtype):
            built.append((n, rank, device, dtype))

    monkeypatch.setattr(solvers, "PivotedCholeskyPreconditioner", Recorded)
    x = torch.randn(40, 2, dtype=torch.float64)
    model = solvers.LatticeGP(plx.RBFLattice(order=1)).double()
    pre = model.preconditioner(x, 5)
    assert type(pre) is Recorded and built == [(40, 5, x.device, torch.float64)]
    assert "_last_preconditioner" not in model.__dict__
    # the snapshot the reuse logic compares is kept in the parameters' own precision
    assert model._hyper_snapshot().dtype == torch.float64
    assert solvers.LatticeGP(plx.RBFLattice(order=1))._hyper_snapshot().dtype == torch.float32


def test_float32_vectors_are_a_type_error():
    """The dtype rule comes before anything that needs a device or a lattice."""
    pre = object.__new__(solvers.LatticePreconditioner64)
    for call in (pre.solve, pre.solve_rows):
        with pytest.raises(TypeError, match="float64"):
            call(torch.zeros(4, 2))
    with pytest.raises(TypeError, match="solve_rows"):
        pre.solve_lattice(torch.zeros(4, 2))
