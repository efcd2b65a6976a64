"""The float64 Lanczos step (plx_lanczos_step_f64, plx_lanczos_work_doubles, plx_lanczos_shape_f64) on the host:
declarations, exports and the signature, the workspace and shape rules, every argument check that returns before any
launch, the module switch, and the routes a CPU double v0 and a library without the calls keep."""
import ctypes
import subprocess

import pytest
import torch

from simplex_gp_amd import _native, training
from tests import solver64

LZ64_SYMBOLS = ("plx_lanczos_work_doubles", "plx_lanczos_shape_f64", "plx_lanczos_step_f64")
PLX_ERR_INVALID = 1
MAX_ROWS = 2_097_152


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


def shape(lib, n):
    span, groups = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.plx_lanczos_shape_f64(n, ctypes.byref(span), ctypes.byref(groups))
    return rc, span.value, groups.value


def test_symbols_declared_and_exported(lib):
    declared = _native.declared_symbols()
    for name in LZ64_SYMBOLS:
        assert name in declared and name in _native._SIGNATURES and name in _native.OPTIONAL_SYMBOLS, name
        assert hasattr(lib, name), name
    assert _native.has_symbols(*LZ64_SYMBOLS)
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in LZ64_SYMBOLS:
        assert f" T {name}\n" in exported, name
    # the feature is detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_signature_is_the_fp32_step():
    sig = _native._SIGNATURES
    assert sig["plx_lanczos_step_f64"] == sig["plx_lanczos_step"]
    assert sig["plx_lanczos_work_doubles"] == sig["plx_lanczos_work_floats"]
    assert lib_max_rows() == 256


def lib_max_rows():
    return int(_native.lib().plx_lanczos_max_rows())


def test_work_doubles(lib):
    for n in (0, -3, MAX_ROWS + 1):
        assert lib.plx_lanczos_work_doubles(n) == -1, n
    ns = (1, 255, 256, 257, 65_536, 65_537, 10 ** 6, MAX_ROWS)
    sizes = [lib.plx_lanczos_work_doubles(n) for n in ns]
    assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    for n, size in zip(ns, sizes):
        rc, span, groups = shape(lib, n)
        assert rc == 0 and size >= 2 * groups * 256 + 256 + groups, (n, size, groups)


def test_shape(lib):
    ns = sorted(set([1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 10 ** 6, MAX_ROWS - 1, MAX_ROWS]
                    + [2 ** k + e for k in range(8, 21) for e in (-1, 0, 1)]))
    last, seen = 0, []
    for n in ns:
        rc, span, groups = shape(lib, n)
        assert rc == 0, n
        if span not in seen:
            seen.append(span)
        assert span * groups >= n and span * (groups - 1) < n, (n, span, groups)
        assert span >= last, (n, span, last)
        last = span
        # static LDS of a workgroup: span doubles of w, next to red[1024] and c[256] (plx_lanczos_kernels.h)
        assert 8 * span <= 49_152 and 8 * span + 8 * 1024 + 8 * 256 <= 65_536, (n, span)
    # the spans the library reports over 1..2,097,152 are the double ladder of the source, the ones its dispatch instantiates
    assert seen == solver64.ladder_spans()["double"], seen
    for n in (0, -3, MAX_ROWS + 1, 2 ** 40):
        rc, span, groups = shape(lib, n)
        assert rc == PLX_ERR_INVALID and (span, groups) == (-1, -1), n
        assert b"plx_lanczos_shape_f64" in lib.plx_last_error()
        assert lib.plx_lanczos_work_doubles(n) == -1
    assert lib.plx_lanczos_shape_f64(3000, None, None) == 0


def _step(lib, p, **kw):
    """A valid call on host addresses but for **kw: basis [2][64] at p, w 512 doubles behind it."""
    at = lambda k: ctypes.c_void_p(p.value + 8 * k)          # noqa: E731
    a = dict(d_q=p, ld=64, d_w=at(512), n=8, i=0, d_alphas=at(600), d_betas=at(640), d_work=at(700))
    a.update(kw)
    return lib.plx_lanczos_step_f64(a["d_q"], a["ld"], a["d_w"], a["n"], a["i"], a["d_alphas"], a["d_betas"], a["d_work"], None)


def test_argument_checks_return_before_any_launch(lib, p):
    """Every PLX_ERR_INVALID of the contract, on host addresses: a launch that followed any of them would fault."""
    who = b"plx_lanczos_step_f64"
    pointers = ("d_q", "d_w", "d_alphas", "d_betas", "d_work")
    base = dict(d_q=0, d_w=512, d_alphas=600, d_betas=640, d_work=700)
    for name in pointers:
        assert _step(lib, p, **{name: None}) == PLX_ERR_INVALID, name
        assert who in lib.plx_last_error() and b"NULL" in lib.plx_last_error(), name
        odd = ctypes.c_void_p(p.value + 8 * base[name] + 4)
        assert _step(lib, p, **{name: odd}) == PLX_ERR_INVALID, name
        assert who in lib.plx_last_error() and b"8-byte" in lib.plx_last_error(), name
    assert _step(lib, p, d_q=ctypes.c_void_p(p.value + 8)) == PLX_ERR_INVALID
    assert who in lib.plx_last_error() and b"16-byte" in lib.plx_last_error()
    assert _step(lib, p, ld=63, n=8) == PLX_ERR_INVALID
    assert who in lib.plx_last_error() and b"multiple of 2" in lib.plx_last_error()
    assert _step(lib, p, ld=64, n=65) == PLX_ERR_INVALID
    assert who in lib.plx_last_error() and b"ld >= n" in lib.plx_last_error()
    for n in (0, -7):
        assert _step(lib, p, n=n) == PLX_ERR_INVALID and who in lib.plx_last_error(), n
    for i in (-1, 256):
        assert _step(lib, p, i=i) == PLX_ERR_INVALID and who in lib.plx_last_error() and b"256" in lib.plx_last_error(), i
    assert _step(lib, p, n=MAX_ROWS + 1, ld=MAX_ROWS + 2) == PLX_ERR_INVALID
    assert who in lib.plx_last_error() and b"2097152 rows" in lib.plx_last_error()
    # d_w inside rows 0..i+1 of the basis: its first element, the last of row i + 1, and w's end reaching into row 0
    at = lambda k: ctypes.c_void_p(p.value + 8 * k)          # noqa: E731
    for w, i in ((p, 0), (at(2 * 64 - 1), 0), (at(3 * 64 + 10), 2)):
        assert _step(lib, p, d_w=w, i=i) == PLX_ERR_INVALID and who in lib.plx_last_error() and b"overlaps" in lib.plx_last_error(), (w, i)
    before = ctypes.c_void_p(p.value - 8 * 4)                # [p - 4, p + 4): the tail of w lies in row 0
    assert _step(lib, p, d_w=before) == PLX_ERR_INVALID and b"overlaps" in lib.plx_last_error()


def test_switch_and_cpu_route():
    assert training.LANCZOS_NATIVE_F64 is True and training.LANCZOS_NATIVE is True
    g = torch.Generator().manual_seed(3)
    n, k = 60, 12
    M = torch.randn(n, n, generator=g, dtype=torch.float64)
    A = M @ M.t() + n * torch.eye(n, dtype=torch.float64)
    v0 = torch.randn(n, generator=g, dtype=torch.float64)
    Q0, T0 = training.lanczos(lambda V: A @ V, v0, k, native=False)
    Q1, T1 = training.lanczos(lambda V: A @ V, v0, k)
    assert Q1.dtype == torch.float64 and torch.equal(Q0, Q1) and torch.equal(T0, T1)


def test_no_symbols_no_native_route(monkeypatch):
    """A library of this ABI without the calls: None for a float64 v0, before anything touches a device."""
    asked = []

    def has(*names):
        asked.append(names)
        return not set(names) & set(LZ64_SYMBOLS)

    monkeypatch.setattr(_native, "has_symbols", has)

    def no_device(V):
        raise AssertionError("the operator was called")

    v0 = torch.ones(16, dtype=torch.float64)
    assert training._lanczos_native(no_device, v0, 4, 32) is None
    assert asked and set(asked[0]) == set(LZ64_SYMBOLS)
