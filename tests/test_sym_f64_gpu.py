"""The transposed and the symmetrised float64 lattice products on the GPU (simplex_gp_amd/csrc/plx_sym_f64.hip):
plx_blur_t_f64 / plx_apply_t_f64, plx_blur_sym_f64 / plx_apply_sym_f64 / plx_apply_affine_sym_f64 and what is built on them.

Yardsticks: tests/sym64 (Kt64: reversed axes with mirrored taps on the structure of Lattice64; Ks64 = (K64 + Kt64) / 2;
tests/test_sym64.py shows on the CPU that Kt64 is the transposed matrix).

Bars, derived, not measured:
  bit contracts   torch.equal: each chain of the dual kernel forms the sums of f64_blur_item in its order, the mean is one
                  rounded sum and an exact halving;
  accuracy        per entry k 2^-52 T with tests/test_f64_gpu.py's k = Lmax + (2 r + 1)(d + 1) + 2 (d + 1) + 8 (the depth of
                  the deepest path), + 2 for the symmetrised sum (one addition, one halving); T the matching terms64;
  adjoint         <K^T a, b> and <a, K b> sum the same n products of |a| terms64(b) size in another order:
                  (n + 4) 2^-52 sum |a| terms64(b), the bar of the fused dot in plx.h;
  solve           true relative residual <= 1e-10, the requirement of tests/test_f64_gpu.py::test_solve_in_double.
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import solvers
from simplex_gp_amd._native import PlxError
from tests.lattice64 import cloud, entry_ratio
from tests.sym64 import Sym64, taps_of

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -52
F64 = torch.float64
PLX_ERR_INVALID, PLX_ERR_STATE = 1, 5
DS, ORDERS, VDS = (1, 2, 3, 8), (0, 1, 2, 3, 4), (1, 2, 3, 12, 130)
CLOUDS = ("gauss1", "isolated", "dup")


def _cases():
    """Every (d, order) pair twice, the widths, tap kinds, clouds, sizes and alignments rotating through it so that every
    width meets every order and every d, both tap kinds meet every order, and every cloud meets both parities of d."""
    out = []
    i = 0
    for a, d in enumerate(DS):
        for b, order in enumerate(ORDERS):
            for rep in range(2):
                vd = VDS[(a + b + 2 * rep + (i // 5) % 2) % len(VDS)]
                out.append((CLOUDS[i % 3], (64, 300)[(i // 3 + rep) % 2], d, order, i % 2 == 1, vd, (i // 2) % 2 == 0))
                i += 1
    for vd in VDS:                                       # every width at the even d with the shared middle axis, order 3
        out.append(("gauss1", 300, 2, 3, True, vd, vd % 2 == 0))
    return out


CASES = _cases()
_OPS, _LATS = {}, {}


def cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def operator(kind, n, d, order, lop):
    key = (kind, n, d, order, lop)
    if key not in _OPS:
        taps = taps_of(order, lop)
        x = cloud(kind, n, d, seed=3 + d + order, coeffs=taps)
        _OPS[key] = (x, Sym64(x, taps), taps)
    return _OPS[key]


def gpu_lattice(kind, n, d, order, lop):
    key = (kind, n, d, order, lop)
    if key not in _LATS:
        x, _, taps = operator(*key)
        _LATS[key] = plx.Lattice().build(cuda(x, np.float32), taps)
    return _LATS[key]


def placed(rows, vd, aligned, fill=None):
    """A contiguous [rows, vd] float64 CUDA tensor whose data pointer is 16-byte aligned, or that plus one double."""
    buf = torch.empty(rows * vd + 2, dtype=F64, device="cuda")
    off = 0 if aligned else 1
    t = buf[off:off + rows * vd].view(rows, vd)
    assert t.data_ptr() % 16 == (0 if aligned else 8)
    if fill is not None:
        t.copy_(fill)
    else:
        t.fill_(float("nan"))
    return t


def depth(lat, extra=0):
    row_ptr = lat.export(nv.ARRAY_ROW_PTR).astype(np.int64)
    lmax = int(np.diff(row_ptr).max())
    d, r = lat.d, lat.order
    return lmax + (2 * r + 1) * (d + 1) + 2 * (d + 1) + 8 + extra


def check_entries(got, op64, v, k, label):
    want, T = op64.apply_staged(v), op64.terms64(v)
    e = entry_ratio(got, want, T)
    print(f"{label}: k = {k}  entry {e:.2e} (bar {k * U2:.2e})")
    assert e <= k * U2, (label, e, k * U2)
    return T


IDS = [f"{c}-n{n}-d{d}-o{o}-{'lop' if l else 'sym'}-vd{vd}-{'al' if al else 'off'}" for c, n, d, o, l, vd, al in CASES]


@pytest.mark.parametrize("kind,n,d,order,lop,vd,aligned", CASES, ids=IDS)
def test_transposed_and_symmetrised_products(kind, n, d, order, lop, vd, aligned):
    x, op, taps = operator(kind, n, d, order, lop)
    lat = gpu_lattice(kind, n, d, order, lop)
    assert lat.m == op.m and lat.order == order and lat.d == d
    label = IDS[CASES.index((kind, n, d, order, lop, vd, aligned))]
    v = np.random.default_rng(vd + 11 * d).standard_normal((n, vd))
    if kind == "isolated":
        v[::2] = 0.0                                   # points no other point reaches: T = 0 there, and so must the products be
    src = placed(n, vd, aligned, cuda(v))
    plain_names = None
    plain = lat.apply(src)
    plain_names = lat.f64_kernels()

    # bit contracts of the blurs, from the staged results
    V = lat.splat(src)
    b = lat.blur(V.clone(), vd=vd).clone()
    bt = lat.blur_t(V.clone(), vd=vd).clone()
    bs = lat.blur_sym(V.clone(), vd=vd)
    assert bs.shape == b.shape
    assert torch.equal(bs, 0.5 * (b + bt)), (label, "blur_sym is not 0.5 (blur + blur_t) to the bit")
    blur_name = lat.sym_f64_kernels()["blur"]
    assert blur_name == ["f64_blur_dual_kernel"], blur_name

    # the products against their staged forms, twice, with no allocation the second time
    got_t = lat.apply_t(src, out=placed(n, vd, aligned)).clone()
    got_s = lat.apply_sym(src, out=placed(n, vd, aligned)).clone()
    names = lat.sym_f64_kernels()
    assert names["blur"] == ["f64_blur_dual_kernel"] and names["splat"] and names["slice"], names
    bytes1 = lat.device_bytes
    assert torch.equal(lat.apply_t(src, out=placed(n, vd, aligned)), got_t), (label, "apply_t not deterministic")
    assert torch.equal(lat.apply_sym(src, out=placed(n, vd, aligned)), got_s), (label, "apply_sym not deterministic")
    assert lat.device_bytes == bytes1, (label, "the second call of a width moved plx_device_bytes")
    assert torch.equal(lat.slice(bt, out=placed(n, vd, aligned), vd=vd), got_t), (label, "apply_t != slice(blur_t(splat))")
    assert torch.equal(lat.slice(bs, out=placed(n, vd, aligned), vd=vd), got_s), (label, "apply_sym != slice(blur_sym(splat))")
    one = torch.tensor([1.0, 0.0], dtype=F64, device="cuda")
    aff = lat.apply_affine(src, one, out=placed(n, vd, aligned), symmetric=True)
    assert torch.equal(aff, got_s), (label, "apply_affine(symmetric=True) with (1, 0) differs from apply_sym")
    # the plain product and what it reports are untouched
    assert lat.f64_kernels() == plain_names and torch.equal(lat.apply(src), plain)

    # accuracy against Kt64 / Ks64
    k = depth(lat)
    Tt = check_entries(got_t.cpu().numpy(), op.kt, v, k, label + " K^T")
    Ts = check_entries(got_s.cpu().numpy(), op, v, k + 2, label + " K_s")
    if kind == "isolated":
        zero = (Ts == 0).all(axis=1) & (Tt == 0).all(axis=1)
        assert zero.sum() >= n // 2 - 1
        assert bool((got_s.cpu().numpy()[zero] == 0).all()) and bool((got_t.cpu().numpy()[zero] == 0).all()), label


ADJOINT = [("gauss1", 300, 3, 2, True, 3), ("dup", 300, 8, 1, True, 2), ("gauss1", 64, 2, 4, True, 1),
           ("gauss1", 300, 1, 3, False, 12)]


@pytest.mark.parametrize("kind,n,d,order,lop,vd", ADJOINT)
def test_adjoint_identities(kind, n, d, order, lop, vd):
    x, op, taps = operator(kind, n, d, order, lop)
    lat = gpu_lattice(kind, n, d, order, lop)
    rng = np.random.default_rng(d + vd)
    a, b = rng.standard_normal((n, vd)), rng.standard_normal((n, vd))
    at, bt = cuda(a), cuda(b)
    bar = (n + 4) * U2 * float((np.abs(a) * op.k.terms64(b)).sum())
    lhs = float((lat.apply_t(at).cpu().numpy() * b).sum())
    rhs = float((a * lat.apply(bt).cpu().numpy()).sum())
    print(f"<K^T a, b> - <a, K b> = {lhs - rhs:.2e} (bar {bar:.2e})")
    assert abs(lhs - rhs) <= bar
    bar_s = (n + 4) * U2 * float((np.abs(a) * op.terms64(b)).sum())
    lhs = float((lat.apply_sym(at).cpu().numpy() * b).sum())
    rhs = float((a * lat.apply_sym(bt).cpu().numpy()).sum())
    print(f"<K_s a, b> - <a, K_s b> = {lhs - rhs:.2e} (bar {bar_s:.2e})")
    assert abs(lhs - rhs) <= bar_s


def test_rebuild_on_the_same_object():
    """The work planes and the kernels follow the build: another build on the same object (other points, other dimension,
    other order) is served from its own tables, and going back gives the first result bit for bit."""
    lat = plx.Lattice()
    outs = []
    for key in (("gauss1", 300, 3, 2, True), ("gauss1", 300, 8, 1, True), ("gauss1", 300, 3, 2, True)):
        x, op, taps = operator(*key)
        lat.build(cuda(x, np.float32), taps)
        for vd in (1, 3):
            v = np.random.default_rng(vd).standard_normal((op.n, vd))
            got = lat.apply_sym(cuda(v))
            check_entries(got.cpu().numpy(), op, v, depth(lat, 2), f"rebuild {key} vd={vd}")
            outs.append(got.clone())
    assert torch.equal(outs[0], outs[4]) and torch.equal(outs[1], outs[5])
    lat.close()


class _Taps:
    """The two calls LatticeFilterGeneral makes on its kernel_fn."""

    def __init__(self, coeffs, deriv):
        self.coeffs, self.deriv = torch.from_numpy(coeffs), torch.from_numpy(deriv)

    def get_coeffs(self):
        return self.coeffs

    def get_deriv_coeffs(self):
        return self.deriv


def test_gradcheck_needs_the_exact_adjoint():
    """torch.autograd.gradcheck of out = K(x) source with respect to `source` (positions fixed): the analytical gradient is
    K^T g.  The reference's K g (py:110-111) is not: with lopsided taps gradcheck fails; with exact_adjoint it passes."""
    n, d, vd = 64, 3, 2
    taps = taps_of(1, True)
    fn = _Taps(taps, np.array([-0.5, 0.0, 0.5], np.float32))
    x = cuda(cloud("gauss1", n, d, seed=2, coeffs=taps))
    src = cuda(np.random.default_rng(0).standard_normal((n, vd))).requires_grad_(True)
    f = lambda s: plx.LatticeFilterGeneral.apply(s, x, fn)        # noqa: E731
    before = plx.LatticeFilterGeneral.exact_adjoint
    try:
        plx.LatticeFilterGeneral.exact_adjoint = False
        assert not torch.autograd.gradcheck(f, (src,), raise_exception=False)
        plx.LatticeFilterGeneral.exact_adjoint = True
        assert torch.autograd.gradcheck(f, (src,))
    finally:
        plx.LatticeFilterGeneral.exact_adjoint = before
        plx.lattice_cache().clear()
    assert before is False


def test_exact_adjoint_with_a_position_gradient():
    """The branch that returns the derivative-tap filter of g today: with the switch on grad_source is K^T g with the
    forward taps there too, and the position gradient is what it was."""
    n, d, vd = 300, 3, 2
    dk = plx.DiscretizedKernelFN(plx.rbf, 1)
    taps = dk.get_coeffs().numpy()
    xn = cloud("gauss1", n, d, seed=4, coeffs=taps)
    g = cuda(np.random.default_rng(1).standard_normal((n, vd)))
    grads = {}
    before = plx.LatticeFilterGeneral.exact_adjoint
    try:
        for on in (False, True):
            plx.LatticeFilterGeneral.exact_adjoint = on
            x = cuda(xn).requires_grad_(True)
            src = cuda(np.random.default_rng(0).standard_normal((n, vd))).requires_grad_(True)
            (plx.LatticeFilterGeneral.apply(src, x, dk) * g).sum().backward()
            grads[on] = (src.grad.clone(), x.grad.clone())
        lat = plx.lattice_cache().get(cuda(xn), taps)
        assert torch.equal(grads[True][0], lat.apply_t(g))
        assert torch.equal(grads[True][1], grads[False][1])
        assert not torch.equal(grads[True][0], grads[False][0])
    finally:
        plx.LatticeFilterGeneral.exact_adjoint = before
        plx.lattice_cache().clear()


def test_solve_on_the_symmetrised_operator():
    """(K_s + 0.1 I) X = B by batched_cg at tol 1e-11, at most 400 iterations, n = 300, d = 2, taps [0.5, 1, 0.5], three
    randn columns: the true relative residual, recomputed on the host with Ks64, is <= 1e-10 (numpy CG on Ks64 needs 65
    iterations).  The plain operator's residual on the same input is printed, not asserted (it stalls)."""
    n, d = 300, 2
    taps = taps_of(1, False)
    x, op, _ = operator("gauss1", n, d, 1, False)
    lat = gpu_lattice("gauss1", n, d, 1, False)
    Ks, K = op.matrix(), op.k.matrix()
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(0), dtype=F64)
    rhs = B.cuda()
    ss = torch.tensor([1.0, 0.1], dtype=F64, device="cuda")
    X, info = solvers.batched_cg(lambda V: lat.apply_affine(V.contiguous(), ss, symmetric=True), rhs, max_iter=400, tol=1e-11)
    Xn, Bn = X.cpu().numpy(), B.numpy()
    res = float(np.linalg.norm((Ks + 0.1 * np.eye(n)) @ Xn - Bn) / np.linalg.norm(Bn))
    Xp, _ = solvers.batched_cg(lambda V: lat.apply_affine(V.contiguous(), ss), rhs, max_iter=400, tol=1e-11)
    resp = float(np.linalg.norm((K + 0.1 * np.eye(n)) @ Xp.cpu().numpy() - Bn) / np.linalg.norm(Bn))
    print(f"solve n = {n}, d = {d}, noise 0.1: K_s true relative residual {res:.2e} in {info.get('iterations')} iterations; "
          f"plain K {resp:.2e}")
    assert X.dtype == F64 and res <= 1e-10, res


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def test_refusals():
    n, d = 300, 3
    taps = taps_of(1, True)
    x = cuda(cloud("gauss1", n, d, seed=1, coeffs=taps), np.float32)
    v = cuda(np.random.default_rng(5).standard_normal((n, 2)))
    lat = plx.Lattice().build(x, taps)
    L = nv.lib()
    # float32 has no transposed or symmetrised form
    ss32 = torch.tensor([1.0, 0.0], device="cuda")
    vals32 = lat.new_values(2)
    for call in (lambda: lat.apply_t(v.float()), lambda: lat.apply_sym(v.float()), lambda: lat.blur_t(vals32, vd=2),
                 lambda: lat.blur_sym(vals32, vd=2), lambda: lat.apply_affine(v.float(), ss32, symmetric=True)):
        with pytest.raises(TypeError, match="float64 only"):
            call()
    # vd = 0, NULL pointers, an aliased d_out for the affine call: PLX_ERR_INVALID, before any GPU work
    out, ss = torch.empty_like(v), torch.tensor([1.0, 0.0], dtype=F64, device="cuda")
    for fn in (L.plx_apply_t_f64, L.plx_apply_sym_f64):
        assert fn(lat._h, _ptr(v), 0, _ptr(out), None) == PLX_ERR_INVALID
        assert fn(lat._h, None, 2, _ptr(out), None) == PLX_ERR_INVALID
        assert fn(lat._h, _ptr(v), 2, None, None) == PLX_ERR_INVALID
        assert fn(None, _ptr(v), 2, _ptr(out), None) == PLX_ERR_INVALID
    assert L.plx_apply_affine_sym_f64(lat._h, _ptr(v), 0, _ptr(out), _ptr(ss), None, None, None) == PLX_ERR_INVALID
    assert L.plx_apply_affine_sym_f64(lat._h, _ptr(v), 2, _ptr(out), None, None, None, None) == PLX_ERR_INVALID
    assert L.plx_apply_affine_sym_f64(lat._h, _ptr(v), 2, _ptr(v), _ptr(ss), None, None, None) == PLX_ERR_INVALID
    assert b"alias" in L.plx_last_error()
    vals = lat.new_values(2, F64)
    work = torch.empty(int(L.plx_blur_sym_work_doubles(lat._h, 2)), dtype=F64, device="cuda")
    res, flag = ctypes.c_void_p(0), ctypes.c_int(0)
    assert L.plx_blur_sym_f64(lat._h, _ptr(vals), _ptr(work), 0, ctypes.byref(res), None) == PLX_ERR_INVALID
    assert L.plx_blur_sym_f64(lat._h, _ptr(vals), None, 2, ctypes.byref(res), None) == PLX_ERR_INVALID
    assert L.plx_blur_sym_f64(lat._h, _ptr(vals), _ptr(work), 2, None, None) == PLX_ERR_INVALID
    assert L.plx_blur_sym_f64(lat._h, _ptr(vals), _ptr(vals), 2, ctypes.byref(res), None) == PLX_ERR_INVALID
    assert L.plx_blur_t_f64(lat._h, _ptr(vals), _ptr(vals), 2, ctypes.byref(flag), None) == PLX_ERR_INVALID
    assert L.plx_blur_t_f64(lat._h, _ptr(vals), _ptr(work), 0, ctypes.byref(flag), None) == PLX_ERR_INVALID
    # the work space: -1 for vd < 1 or an unbuilt lattice, at most 3 m stride
    assert L.plx_blur_sym_work_doubles(lat._h, 0) == -1
    assert 0 < L.plx_blur_sym_work_doubles(lat._h, 3) <= 3 * lat.m * plx.Lattice.values_stride(3, F64)
    fresh = plx.Lattice()
    assert L.plx_blur_sym_work_doubles(fresh._h, 2) == -1
    assert L.plx_apply_sym_f64(fresh._h, _ptr(v), 2, _ptr(out), None) == PLX_ERR_STATE
    fresh.close()
    lat.close()
    # a build that replayed the reference's table growth: its neighbour table is not symmetric
    nv.check(L.plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        lat = plx.Lattice().build(x, taps)
    finally:
        nv.check(L.plx_tune(b"reference_growth", 0), "plx_tune")
    assert lat.reference_growth_info()["replayed"]
    for call in (lambda: lat.apply_t(v), lambda: lat.apply_sym(v), lambda: lat.apply_affine(v, ss, symmetric=True)):
        with pytest.raises(PlxError) as err:
            call()
        assert err.value.code == PLX_ERR_STATE and "reference_growth" in str(err.value)
    lat.close()


def test_first_call_under_capture_is_refused():
    rng = np.random.default_rng(3)
    n, d = 2000, 3
    lat = plx.Lattice().build(cuda(rng.standard_normal((n, d)), np.float32), taps_of(1, True))
    v = cuda(rng.standard_normal((n, 4)))
    out = torch.empty_like(v)
    lat.apply(v)                                            # the plain workspace exists; the two further planes do not
    before = lat.device_bytes
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(PlxError, match="captured") as err:
        with torch.cuda.graph(graph, stream=s):
            lat.apply_sym(v, out=out)
    assert err.value.code == PLX_ERR_STATE and lat.device_bytes == before
    del graph
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        eager = lat.apply_sym(v, out=out).clone()
        first = lat.device_bytes
        assert first >= before + 2 * lat.m * 4 * 8
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        out.zero_()
        with torch.cuda.graph(graph, stream=s):
            lat.apply_sym(v, out=out)
        graph.replay()
        s.synchronize()
        assert torch.equal(out, eager) and lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


def test_model_and_operator_switches():
    """LatticeGP.symmetric_f64 reaches khat_in_lattice_rows (its closure is s apply_sym(V) + sigma^2 V) and khat_solve;
    SquareLazyLattice(symmetrized=True) multiplies by K_s.  Both switches are off by default."""
    n, d = 300, 3
    assert solvers.LatticeGP.symmetric_f64 is False and plx.LatticeFilterGeneral.exact_adjoint is False
    x = cuda(np.random.default_rng(2).standard_normal((n, d)))
    V = cuda(np.random.default_rng(3).standard_normal((n, 2)))
    try:
        model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).double().cuda()
        with torch.no_grad():
            s, noise = model.outputscale, model.noise
            with model.khat_in_lattice_rows(x) as (mm, _, _):
                plain = mm(V).clone()
            model.symmetric_f64 = True
            with model.khat_in_lattice_rows(x) as (mm, to_rows, from_rows):
                assert to_rows(V) is V and from_rows(V) is V
                got = mm(V).clone()
            ref = x / model.kernel.lengthscale.detach()
            lat = plx.lattice_cache().get(ref.contiguous(), model.kernel.dkernel_fn.get_coeffs())
            want = s * lat.apply_sym(V) + noise * V
            assert float((got - want).abs().max()) <= 8 * U2 * float(want.abs().max())
            assert not torch.allclose(got, plain, rtol=0, atol=1e-6)
            sol = model.khat_solve(x, V, tol=1e-11, max_iter=400)
            sol = sol[0] if isinstance(sol, tuple) else sol
            res = float((s * lat.apply_sym(sol) + noise * sol - V).norm() / V.norm())
            print(f"khat_solve on s K_s + sigma^2 I: residual {res:.2e}")
            assert res <= 1e-10
            k = model.kernel
            sq = plx.SquareLazyLattice(ref, dkernel=k.dkernel_fn, symmetrized=True)
            assert sq._transpose_nonbatch() is sq
            assert torch.equal(sq.matmul(V), lat.apply_sym(V))
            assert torch.equal(plx.SquareLazyLattice(ref, dkernel=k.dkernel_fn).matmul(V), lat.apply(V))
    finally:
        plx.lattice_cache().clear()
