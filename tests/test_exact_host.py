"""The exact kernel MVM on the host: the C ABI's argument checks (all made before any GPU work), the workspace bound,
the Python error paths that need no device, exact_twin and mvm_error's formulas."""
import ctypes
import math

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_float * 1024)()                   # host memory: every call below returns before a launch could reach it
    p = ctypes.cast(buf, ctypes.c_void_p)
    p._keep = buf
    return p


def test_exact_symbols_and_version(lib):
    for name in ("plx_exact_work_bytes", "plx_exact_splits", "plx_exact_mvm", "plx_exact_grad"):
        assert name in _native.declared_symbols() and name in _native._SIGNATURES
    assert lib.plx_version().decode().startswith("libplx 0.9.")
    assert _native.ABI_VERSION == (0, 9)


def test_exact_mvm_argument_checks(lib, p):
    W = 1 << 26
    ok = dict(x1=p, n1=64, x2=p, n2=64, d=3, prof=0, v=p, t=1, out=p, work=p, wb=W)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.plx_exact_mvm(a["x1"], a["n1"], a["x2"], a["n2"], a["d"], a["prof"], a["v"], a["t"], a["out"],
                                 a["work"], a["wb"], None)

    for name in ("x1", "x2", "v", "out", "work"):
        assert call(**{name: None}) == 1 and b"NULL" in lib.plx_last_error(), name
    assert call(d=0) == 4 and b"d = 0" in lib.plx_last_error()
    assert call(d=33) == 4 and b"d = 33" in lib.plx_last_error()
    assert call(prof=4) == 1 and b"profile" in lib.plx_last_error()
    assert call(prof=-1) == 1
    assert call(t=0) == 1 and b"t = 0" in lib.plx_last_error()
    assert call(n1=0) == 1 and call(n2=0) == 1 and call(n1=1 << 31) == 1 and call(n2=-5) == 1
    need = lib.plx_exact_work_bytes(64, 64, 3, 1)
    assert need > 0
    assert call(wb=need - 1) == 1 and b"workspace" in lib.plx_last_error()


def test_exact_grad_argument_checks(lib, p):
    W = 1 << 26
    ok = dict(x1=p, n1=64, x2=p, n2=64, d=3, prof=2, g=p, v=p, t=5, out=p, work=p, wb=W)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.plx_exact_grad(a["x1"], a["n1"], a["x2"], a["n2"], a["d"], a["prof"], a["g"], a["v"], a["t"],
                                  a["out"], a["work"], a["wb"], None)

    for name in ("x1", "x2", "g", "v", "out", "work"):
        assert call(**{name: None}) == 1 and b"NULL" in lib.plx_last_error(), name
    assert call(d=0) == 4 and call(d=33) == 4
    assert call(prof=7) == 1 and b"profile" in lib.plx_last_error()
    assert call(t=0) == 1
    assert call(wb=lib.plx_exact_work_bytes(64, 64, 3, 5) - 1) == 1 and b"workspace" in lib.plx_last_error()


def test_exact_work_bytes_limits_and_monotone(lib):
    assert lib.plx_exact_work_bytes(0, 10, 3, 1) == -1 and lib.plx_exact_work_bytes(10, 0, 3, 1) == -1
    assert lib.plx_exact_work_bytes(10, 10, 0, 1) == -1 and lib.plx_exact_work_bytes(10, 10, 33, 1) == -1
    assert lib.plx_exact_work_bytes(10, 10, 3, 0) == -1 and lib.plx_exact_work_bytes(1 << 31, 10, 3, 1) == -1
    sizes_n = [1, 2, 7, 8, 255, 256, 257, 777, 3001, 5000, 65536, 100_000, 262_145, 1_000_000, 2_049_280, (1 << 31) - 1]
    ds, ts = [1, 3, 8, 18, 32], [1, 3, 11, 64, 257, 4096]
    for n2 in [1, 511, 512, 5000, 200_000, 2_000_000]:
        for d in ds:
            for t in ts:
                w = [lib.plx_exact_work_bytes(n1, n2, d, t) for n1 in sizes_n]
                assert all(b > 0 for b in w) and w == sorted(w), (n2, d, t, w)
    for n1 in sizes_n[::3]:
        w = [lib.plx_exact_work_bytes(n1, n2, 8, 11) for n2 in sizes_n]
        assert w == sorted(w), (n1, w)
        w = [lib.plx_exact_work_bytes(n1, 5000, d, 11) for d in range(1, 33)]
        assert w == sorted(w), (n1, w)
        w = [lib.plx_exact_work_bytes(n1, 5000, 8, t) for t in ts]
        assert w == sorted(w), (n1, w)
    assert max(lib.plx_exact_work_bytes(n, n, 32, 4096) for n in sizes_n) <= 16 << 20


def test_exact_splits_limits_and_workspace(lib):
    """the split count is refused exactly where the workspace bound is, and its slabs (n1 max(d, t) floats each) fit the
    workspace at every size"""
    assert lib.plx_exact_splits(0, 10, 3, 1) == -1 and lib.plx_exact_splits(10, 0, 3, 1) == -1
    assert lib.plx_exact_splits(10, 10, 0, 1) == -1 and lib.plx_exact_splits(10, 10, 33, 1) == -1
    assert lib.plx_exact_splits(10, 10, 3, 0) == -1 and lib.plx_exact_splits(1 << 31, 10, 3, 1) == -1
    assert lib.plx_exact_splits(10, 1 << 31, 3, 1) == -1 and lib.plx_exact_splits(-1, 10, 3, 1) == -1
    assert lib.plx_exact_splits(4096, 4096, 3, 1) == 8 and lib.plx_exact_splits(8, 200_000, 8, 11) == 390
    assert lib.plx_exact_splits(64, 511, 3, 1) == 1 and lib.plx_exact_splits(1_000_000, 1_000_000, 3, 1) == 1
    sizes = [1, 7, 8, 255, 256, 257, 3001, 65536, 262_145, 524_288, 524_289, 2_049_280, (1 << 31) - 1]
    for n1 in sizes:
        for n2 in sizes:
            for d, t in ((1, 1), (3, 1), (32, 1), (3, 11), (8, 64), (18, 257), (32, 4096), (1, 5_000_000)):
                s = lib.plx_exact_splits(n1, n2, d, t)
                assert 1 <= s <= 1024 and (s == 1 or s <= max(1, n2 // 512)), (n1, n2, d, t, s)
                if s > 1:
                    assert 4 * s * n1 * max(d, t) <= lib.plx_exact_work_bytes(n1, n2, d, t), (n1, n2, d, t, s)


def test_exact_matmul_has_no_cpu_path():
    x = torch.randn(10, 3)
    v = torch.randn(10, 2)
    with pytest.raises(ValueError, match="no CPU path"):
        plx.exact_matmul(x, x, v, "rbf")
    with pytest.raises(ValueError, match="unknown profile"):
        plx.exact_matmul(x, x, v, "laplace")
    with pytest.raises(ValueError, match="no CPU path"):
        plx.RBFExact()(x, x) @ v


def test_exact_kernel_factories():
    assert plx.RBFExact().profile == "rbf"
    assert [plx.MaternExact(nu=nu).profile for nu in (0.5, 1.5, 2.5)] == ["matern12", "matern32", "matern52"]
    with pytest.raises(ValueError):
        plx.MaternExact(nu=3.5)
    k = plx.RBFExact(ard_num_dims=4)
    assert tuple(k.lengthscale.shape) == (1, 4)
    x = torch.randn(7, 4)
    assert torch.equal(k(x, x, diag=True), torch.ones(7))
    K = k(x, x)
    assert tuple(K.shape) == (7, 7) and torch.equal(K.diag(), torch.ones(7))
    Kr = k(x[:3], x)
    assert tuple(Kr.shape) == (3, 7) and tuple(Kr.t().shape) == (7, 3)


def test_exact_twin_of_the_lattice_factories():
    k = plx.RBFLattice(order=1)
    k.lengthscale = 0.8
    t = plx.exact_twin(k)
    assert isinstance(t, plx.ExactKernel) and t.profile == "rbf"
    assert torch.allclose(t.lengthscale, k.lengthscale)
    assert plx.exact_twin(plx.BilateralKernel()).profile == "rbf"
    m = plx.MaternLattice(nu=1.5, ard_num_dims=3)
    m.lengthscale = torch.tensor([[0.5, 1.0, 2.0]])
    tm = plx.exact_twin(m)
    assert tm.profile == "matern32" and torch.allclose(tm.lengthscale, m.lengthscale) and tm.ard_num_dims == 3
    assert plx.exact_twin(plx.MaternLattice(nu=2.5)).profile == "matern52"
    bare = plx.LatticeAccelerated(lambda d2: (-d2).exp(), order=1)
    with pytest.raises(ValueError, match="profile"):
        plx.exact_twin(bare)


def test_mvm_error_formulas():
    g = torch.Generator().manual_seed(3)
    b = torch.randn(500, 1, generator=g) + 2.0
    a = 1.3 * b + 0.05 * torch.randn(500, 1, generator=g)
    e = plx.mvm_error(a, b)
    ad, bd = a.double().flatten(), b.double().flatten()
    s = ad / (ad / bd).mean()
    want_rel = math.sqrt(((bd - s) ** 2).mean()) / (math.sqrt((bd ** 2).mean()) + math.sqrt((s ** 2).mean()))
    assert e["rel_err"] == pytest.approx(want_rel, rel=1e-12)
    assert e["cos_err"] == pytest.approx(float(ad @ bd / (ad.norm() * bd.norm())), rel=1e-12)
    assert e["rel_l2"] == pytest.approx(float((ad - bd).norm() / bd.norm()), rel=1e-12)
    same = plx.mvm_error(b, b)
    assert same["rel_err"] == 0.0 and same["rel_l2"] == 0.0 and same["cos_err"] == pytest.approx(1.0, abs=1e-15)
    # the mean-ratio rescale removes a pure scale
    assert plx.mvm_error(2.5 * b, b)["rel_err"] < 1e-7                    # (2.5 b is rounded to fp32)
