"""The float64 product (plx_apply_f64 and its three stages, simplex_gp_amd/csrc/plx_f64.hip) on the GPU.

Yardstick: tests/lattice64.Lattice64, the float64 operator assembled with scipy from the CPU oracle's structure.  The native
fp64 product is the same operator (the build's fp32 weights and taps converted exactly, every sum in double, one division
by 1 + 2^-d), so the two differ by the rounding of double sums taken in different orders.

The bar is derived per case, not measured: k 2^-52 of T (T = terms64, the size of the terms an entry sums), with
    k = Lmax + (2 r + 1)(d + 1) + 2 (d + 1) + 8
the additions and multiplications along the deepest path -- Lmax corners in the longest vertex row (from the exported
PLX_ARRAY_ROW_PTR), 2 r + 1 taps on each of d + 1 axes, d + 1 corners in the slice with their weights, the division and
slack for the conversions -- with the unit roundoff 2^-53 counted once for each side of the comparison.  rel-L2 gets the
same k 2^-52 times ||T|| / ||want|| of the case.  Measured worst per stage family (pytest -s prints them; DESIGN.md section
14 lists them): see family_report().

The fp32 product is then judged against the NATIVE fp64 product with the bars tests/test_forward_fp64.py uses (ENTRY, REL),
on the same cases and once at the headline shape N = 1e6, d = 8 -- the full-size comparison that the CPU yardstick cannot
make; there T is the fp64 product of |v| on the device (weights and taps are non-negative, so that is terms64).
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import solvers
from simplex_gp_amd._native import PlxError
from tests.lattice64 import Lattice64, backward64, cloud, entry_ratio, grad_x_ratios, rel_l2
from tests.test_forward_fp64 import ENTRY, REL

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -52
PLX_ERR_STATE = 5

V1 = ("f64_splat_v1_kernel", "f64_blur_v1_kernel", "f64_slice_v1_kernel")
CHUNK = ("f64_splat_chunk_kernel", "f64_blur_chunk_kernel", "f64_slice_chunk_kernel")
WIDE = ("f64_splat_wide_kernel", "f64_blur_chunk_kernel", "f64_slice_wide_kernel")
FAMILIES = (V1, CHUNK, WIDE)


def expect(vd):
    """The family plx_f64.hip picks: by the row width alone (chunks of two doubles)."""
    nch = (vd + 1) // 2
    return V1 if vd == 1 else CHUNK if nch <= 64 else WIDE


def gauss_taps(order):
    half = np.exp(-0.5 * (np.arange(1, order + 1) * 0.7) ** 2)
    return np.concatenate([half[::-1], [1.0], half]).astype(np.float32)


# name -> (cloud, n, d, order): d in {1, 3, 8, 18}, orders 0..3, every cloud of tests/lattice64
LATTICES = {
    "d1": ("gauss1", 3001, 1, 1),
    "d3": ("gauss1", 3000, 3, 2),
    "d8": ("gauss1", 3000, 8, 3),
    "d18": ("gauss1", 1500, 18, 1),
    "coarse-o0": ("gauss0.3", 4000, 3, 0),       # taps of length 1: the blur multiplies by the centre tap d + 1 times
    "d8-o0": ("gauss3", 2000, 8, 0),
    "gauss3": ("gauss3", 2000, 8, 1),
    "simplex": ("simplex", 1500, 3, 1),          # d + 1 vertex rows of n corners each
    "isolated": ("isolated", 1000, 3, 2),
    "dup": ("dup", 2000, 8, 2),
    "grid": ("grid", 2000, 3, 3),
    "d24": ("gauss1", 600, 24, 1),               # d + 1 > 20: the slices' run-time form; its own two cases, not the rotation
}
VDS = (1, 2, 3, 4, 11, 12, 101, 520)


def _cases():
    out = []
    for i, lname in enumerate(l for l in LATTICES if l != "d24"):
        for j in range(3):                                   # three widths per lattice, rotating through all of them
            vd = VDS[(3 * i + j) % len(VDS)]
            out.append((lname, vd, (i + j) % 2 == 0))
    for vd in VDS:                                           # every width, aligned and offset, at one lattice
        for aligned in (True, False):
            if ("d8", vd, aligned) not in out:
                out.append(("d8", vd, aligned))
    for vd in (1, 12, 520):                                  # every family on the sparse high-dimensional lattice
        if ("d18", vd, True) not in out:
            out.append(("d18", vd, True))
    out += [("d24", 1, True), ("d24", 12, False)]
    return out


CASES = _cases()
_OPS, _LATS = {}, {}


def operator(lname):
    """(x, Lattice64, taps) of a named lattice, built once for the module."""
    if lname not in _OPS:
        kind, n, d, order = LATTICES[lname]
        taps = gauss_taps(order)
        x = cloud(kind, n, d, seed=11, coeffs=taps)
        _OPS[lname] = (x, Lattice64(x, taps), taps)
    return _OPS[lname]


def gpu_lattice(lname):
    if lname not in _LATS:
        x, _, taps = operator(lname)
        _LATS[lname] = plx.Lattice().build(cuda(x), taps)
    return _LATS[lname]


def cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def placed(rows, vd, aligned, fill=None):
    """A contiguous [rows, vd] float64 CUDA tensor whose data pointer is 16-byte aligned, or that plus one double."""
    buf = torch.empty(rows * vd + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = 0 if aligned else 1
    t = buf[off:off + rows * vd].view(rows, vd)
    assert t.is_contiguous() and t.data_ptr() % 16 == (0 if aligned else 8)
    if fill is not None:
        t.copy_(fill)
    else:
        t.fill_(float("nan"))
    return t


def depth(lat, extra=0):
    """k of the module docstring for a built lattice."""
    row_ptr = lat.export(nv.ARRAY_ROW_PTR).astype(np.int64)
    lmax = int(np.diff(row_ptr).max())
    d, r = lat.d, lat.order
    return lmax + (2 * r + 1) * (d + 1) + 2 * (d + 1) + 8 + extra


WORST = {}        # family -> [entry ratio / (k 2^-52), rel-L2 / its bar, entry ratio, cases]
WORST32 = {}      # fp32 family -> [entry ratio, rel-L2, cases]
REACHED = set()


def family_of(lat):
    k = lat.f64_kernels()
    return ("+".join(k["splat"]), "+".join(k["blur_axis"]), "+".join(k["slice"]))


def check64(lat, l64, got, v, label, fam):
    want, T = l64.apply_staged(v), l64.terms64(v)
    k = depth(lat)
    e, r = entry_ratio(got, want, T), rel_l2(got, want)
    rbar = k * U2 * float(np.linalg.norm(T)) / max(float(np.linalg.norm(want)), 1e-300)
    w = WORST.setdefault(fam, [0.0, 0.0, 0.0, 0])
    w[0], w[1], w[2], w[3] = max(w[0], e / (k * U2)), max(w[1], r / rbar), max(w[2], e), w[3] + 1
    print(f"{label}: k = {k}  entry {e:.2e} (bar {k * U2:.2e})  rel-L2 {r:.2e} (bar {rbar:.2e})  {fam[0]} {fam[2]}")
    assert e <= k * U2, (label, "entry ratio", e, k * U2)
    assert r <= rbar, (label, "rel-L2", r, rbar)
    return T


def check32(lat, out32, out64, T, label):
    """The fp32 product against the native fp64 one, with the bars of tests/test_forward_fp64.py."""
    k = lat.stage_kernels()
    fam = ("+".join(k["splat"]), "+".join(k["blur_axis"]), "+".join(k["slice"]))
    e, r = entry_ratio(out32, out64, T), rel_l2(out32, out64)
    w = WORST32.setdefault(fam, [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], e), max(w[1], r), w[2] + 1
    print(f"{label}: fp32 against native fp64: entry {e:.2e} rel-L2 {r:.2e}  {fam}")
    assert e <= ENTRY and r <= REL, (label, "fp32 against native fp64", e, r)


@pytest.mark.parametrize("lname,vd,aligned", CASES, ids=[f"{a}-vd{b}-{'al' if c else 'off'}" for a, b, c in CASES])
def test_f64_product_against_lattice64(lname, vd, aligned):
    x, l64, taps = operator(lname)
    kind, n, d, order = LATTICES[lname]
    lat = gpu_lattice(lname)
    assert lat.m == l64.m and lat.order == order
    label = f"{lname} vd={vd} {'aligned' if aligned else 'offset'}"
    v = np.random.default_rng(vd + 7).standard_normal((n, vd))
    if kind == "isolated":
        v[::2] = 0.0                                   # points no other point reaches: T = 0 there, and so must the product be
    src = placed(n, vd, aligned, cuda(v, np.float64))
    # item 2: two calls are bit-equal; the second call of a width leaves plx_device_bytes alone
    got = lat.apply(src, out=placed(n, vd, aligned)).clone()
    bytes1 = lat.device_bytes
    again = lat.apply(src, out=placed(n, vd, aligned))
    assert lat.device_bytes == bytes1, (label, "the second fp64 call of a width moved plx_device_bytes")
    assert torch.equal(got, again), (label, "not deterministic")
    fam = family_of(lat)
    assert fam == expect(vd), (label, fam)
    REACHED.update(fam)
    # item 1: against Lattice64
    T = check64(lat, l64, got.cpu().numpy(), v, label, fam)
    if kind == "isolated":
        zero = (T == 0).all(axis=1)
        assert zero.sum() >= n // 2 - 1 and bool((got.cpu().numpy()[zero] == 0).all()), label
    # item 2: the staged calls give the bits of apply
    values = lat.splat(src)
    assert values.dtype == torch.float64 and values.shape == (lat.m, plx.Lattice.values_stride(vd, torch.float64))
    staged = lat.slice(lat.blur(values, vd=vd), out=placed(n, vd, aligned), vd=vd)
    assert torch.equal(staged, got), (label, "splat + blur + slice differs from apply")
    assert family_of(lat) == fam
    # item 3: the fp32 path with fp32 inputs against the native fp64 product of the same inputs
    v32 = v.astype(np.float32)
    out32 = lat.apply(cuda(v32)).cpu().numpy()
    out64 = lat.apply(cuda(v32, np.float64)).cpu().numpy()
    check32(lat, out32, out64, l64.terms64(v32), label)


def test_rebuild_on_the_same_object():
    """The fp64 tables belong to a build: a second build on the same object (other points, other dimension) is served from
    its own corner table, and going back gives the first result bit for bit."""
    lat = plx.Lattice()
    outs = []
    for lname in ("d3", "d8", "d3"):
        x, l64, taps = operator(lname)
        lat.build(cuda(x), taps)
        for vd in (1, 3):
            v = np.random.default_rng(vd).standard_normal((l64.n, vd))
            got = lat.apply(cuda(v, np.float64))
            check64(lat, l64, got.cpu().numpy(), v, f"rebuild {lname} vd={vd}", family_of(lat))
            outs.append(got.clone())
    assert torch.equal(outs[0], outs[4]) and torch.equal(outs[1], outs[5])


def test_headline_fp32_against_native_fp64():
    """N = 1e6, d = 8, order 1 (the headline build: x ~ N(0, I) from seed 1234), vd in {1, 12}: every entry of the fp32
    product against the fp64 product on the same lattice, T computed on the device as the fp64 product of |v|."""
    n, d = 1_000_000, 8
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=g).cuda()
    taps = np.array([0.34608543, 1.0, 0.34608543], np.float32)
    lat = plx.Lattice().build(x, taps)
    for vd in (1, 12):
        v = torch.randn(n, vd, generator=g).cuda()
        out32 = lat.apply(v).double()
        out64 = lat.apply(v.double())
        T = lat.apply(v.double().abs())
        assert family_of(lat) == expect(vd)
        assert bool(torch.isfinite(out64).all()) and bool((T > 0).all())
        e = float(((out32 - out64).abs() / T).max())
        r = float((out32 - out64).norm() / out64.norm())
        print(f"headline N = 1e6 d = 8 vd = {vd}: fp32 against native fp64: entry {e:.2e} rel-L2 {r:.2e} "
              f"{lat.stage_kernels()}")
        assert e <= ENTRY and r <= REL, (vd, e, r)
    lat.close()


def deriv_and_taps(order=1):
    dk = plx.DiscretizedKernelFN(plx.rbf, order)
    return dk, dk.get_coeffs().numpy(), dk.get_deriv_coeffs().numpy()


@pytest.mark.parametrize("kind,d,L", [("gauss1", 3, 2), ("gauss1", 8, 3), ("isolated", 3, 2)])
def test_autograd_in_double(kind, d, L):
    """V.grad and x.grad of (K(x) V . G).sum() in float64 against lattice64.backward64.  grad_source is the native fp64
    product on the derivative-tap lattice (py:123), under the bar of the product; the position gradient is a contraction of
    4 (L + 1) more terms per entry around it: k' = k + 4 (L + 1)."""
    n = 701
    dk, taps, dtaps = deriv_and_taps(1)
    x = cloud(kind, n, d, seed=d, coeffs=taps)
    rng = np.random.default_rng(d * L)
    v, w = rng.standard_normal((n, L)), rng.standard_normal((n, L))
    lat64 = Lattice64(x, dtaps)
    gx64, gs64, T = backward64(w, v, x, dtaps, lattice=lat64)
    try:
        xt = cuda(x, np.float64).requires_grad_(True)
        vt = cuda(v, np.float64).requires_grad_(True)
        out = plx.LatticeFilterGeneral.apply(vt, xt, dk)
        assert out.dtype == torch.float64
        (out * cuda(w, np.float64)).sum().backward()
        assert xt.grad.dtype == torch.float64 and vt.grad.dtype == torch.float64
        fwd = Lattice64(x, taps)
        hip = plx.lattice_cache().get(xt.detach(), dtaps)            # the derivative-tap lattice the backward ran on
        k = depth(hip)
        kf = depth(plx.lattice_cache().get(xt.detach(), taps))
        e = entry_ratio(out.detach().cpu().numpy(), fwd.apply_staged(v), fwd.terms64(v))
        assert e <= kf * U2, ("forward", kind, d, L, e)
        es = entry_ratio(vt.grad.cpu().numpy(), gs64, lat64.terms64(w))
        kx = k + 4 * (L + 1)
        terms, rel = grad_x_ratios(xt.grad.cpu().numpy(), gx64, T)
        print(f"autograd double {kind} d={d} L={L}: V.grad entry {es:.2e} (bar {k * U2:.2e})  x.grad / ||T|| {terms:.2e} "
              f"(bar {kx * U2:.2e})  rel-L2 {rel}")
        assert es <= k * U2, ("V.grad", kind, d, L, es)
        assert terms <= kx * U2, ("x.grad", kind, d, L, terms)
        if kind == "isolated":                               # the true gradient vanishes: what is left is rounding of T
            assert float(np.abs(xt.grad.cpu().numpy()).max()) <= kx * U2 * float(T.max())
    finally:
        plx.lattice_cache().clear()


def true_residual(K, X, B):
    R = (K + np.eye(K.shape[0])) @ X - B
    return float(np.linalg.norm(R) / np.linalg.norm(B))


def test_solve_in_double():
    """The experiment that motivates the feature: (K + 1.0 I) X = B by batched_cg at tol 1e-11 through the native fp64
    operator; the true relative residual, recomputed on the CPU with the yardstick matrix, must be <= 1e-10 (the yardstick
    matrix alone reaches 8.9e-12 in 168 iterations on the CPU).  The same solve in float32 is printed, not asserted (it
    stalled at 3.4e-6 on the CPU)."""
    n, d = 2000, 3
    taps = np.array([0.5, 1.0, 0.5], np.float32)
    x = cloud("gauss1", n, d, seed=1)
    K = Lattice64(x, taps).matrix()
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    lat = plx.Lattice().build(cuda(x), taps)
    res = {}
    for dtype in (torch.float64, torch.float32):
        rhs = B.to(dtype).cuda()
        X = solvers.batched_cg(lambda V: lat.apply(V.contiguous()) + 1.0 * V, rhs, max_iter=1000, tol=1e-11)
        X = X[0] if isinstance(X, tuple) else X
        assert X.dtype == dtype
        res[dtype] = true_residual(K, X.double().cpu().numpy(), B.numpy())
        print(f"solve (K + I) X = B, n = {n}, d = {d}, {dtype}: true relative residual {res[dtype]:.2e}")
    assert res[torch.float64] <= 1e-10, res
    lat.close()


def _raw_apply_f64(lat, src, out, stream=None):
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    return nv.lib().plx_apply_f64(lat._h, ctypes.c_void_p(src.data_ptr()), src.shape[1], ctypes.c_void_p(out.data_ptr()), s)


def test_memory_and_capture():
    rng = np.random.default_rng(3)
    n, d = 20000, 4
    taps = gauss_taps(1)
    x = cuda(rng.standard_normal((n, d)))
    lat = plx.Lattice().build(x, taps)
    v32 = cuda(rng.standard_normal((n, 4)))
    lat.apply(v32)
    after_build = lat.device_bytes
    for _ in range(3):                                      # fp32 use never allocates the fp64 workspace
        lat.apply(v32)
        lat.apply(v32[:, :1].contiguous())
    fp32_bytes = lat.device_bytes
    lat.apply(v32)
    assert lat.device_bytes == fp32_bytes >= after_build
    # a first fp64 call under capture is refused (PLX_ERR_STATE), and the stream survives
    v = v32.double()
    out = torch.empty_like(v)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(PlxError, match="captured") as err:
        with torch.cuda.graph(graph, stream=s):
            lat.apply(v, out=out)
    assert err.value.code == PLX_ERR_STATE
    assert lat.device_bytes == fp32_bytes
    del graph
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert torch.isfinite(lat.apply(v32)).all()         # the stream and the lattice still work
        # the first fp64 call allocates: two planes of doubles and, here, nothing the fp32 calls had not built already
        # except the corner table and its row pointer
        eager = lat.apply(v, out=out).clone()
        first = lat.device_bytes
        assert first >= fp32_bytes + 2 * lat.m * 4 * 8
        lat.apply(v, out=out)
        assert lat.device_bytes == first                    # the second call of a width: no allocation
        # captured after one eager call, the product replays to the same bits -- also on a new right-hand side
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        out.zero_()
        with torch.cuda.graph(graph, stream=s):
            lat.apply(v, out=out)
        graph.replay()
        s.synchronize()
        assert torch.equal(out, eager)
        v2 = cuda(rng.standard_normal((n, 4)), np.float64)
        want2 = lat.apply(v2).clone()
        v.copy_(v2)
        graph.replay()
        s.synchronize()
        assert torch.equal(out, want2)
        assert lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


def test_refusals():
    rng = np.random.default_rng(5)
    n, d = 3000, 3
    taps = gauss_taps(1)
    x = cuda(rng.standard_normal((n, d)))
    v = cuda(rng.standard_normal((n, 2)), np.float64)
    # one shard of two: the fp64 product serves plain single-shard builds only
    lat = plx.Lattice().build(x, taps, shard=(0, 2))
    own = v[:lat.n_owned].contiguous()
    with pytest.raises(PlxError) as err:
        lat.apply(own)
    assert err.value.code == PLX_ERR_STATE and "shard" in str(err.value)
    values = torch.zeros((lat.m, 2), dtype=torch.float64, device="cuda")
    for call in (lambda: lat.splat(own), lambda: lat.blur(values, vd=2), lambda: lat.slice(values, vd=2)):
        with pytest.raises(PlxError) as err:
            call()
        assert err.value.code == PLX_ERR_STATE
    lat.close()
    # a build that replayed the reference's table growth
    nv.check(nv.lib().plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        lat = plx.Lattice().build(x, taps)
    finally:
        nv.check(nv.lib().plx_tune(b"reference_growth", 0), "plx_tune")
    assert lat.reference_growth_info()["replayed"]
    with pytest.raises(PlxError) as err:
        lat.apply(v)
    assert err.value.code == PLX_ERR_STATE and "reference_growth" in str(err.value)
    assert torch.isfinite(lat.apply(v.float())).all()       # the fp32 product goes on serving it
    lat.close()
    # an unbuilt lattice, and misaligned value rows
    lat = plx.Lattice()
    assert _raw_apply_f64(lat, v, torch.empty_like(v)) == PLX_ERR_STATE and b"not built" in nv.lib().plx_last_error()
    lat.build(x, taps)
    buf = torch.zeros(lat.m * 2 + 2, dtype=torch.float64, device="cuda")
    rc = nv.lib().plx_splat_f64(lat._h, ctypes.c_void_p(v.data_ptr()), 2, ctypes.c_void_p(buf.data_ptr() + 8), None)
    assert rc == 1 and b"16-byte" in nv.lib().plx_last_error()
    lat.close()


def test_boundary_in_double():
    """filter, the extension's filter / LatticeHandle and the operator classes take float64 pairs; all of them give the bits
    of Lattice.apply on the lattice of the rounded positions."""
    ext = plx.torch_ext.load()                 # the one way the extension is loaded: a second import registers its types twice
    x, l64, taps = operator("d3")
    n = l64.n
    v = np.random.default_rng(1).standard_normal((n, 3))
    xt, vt, ct = cuda(x, np.float64), cuda(v, np.float64), torch.from_numpy(taps)
    want = gpu_lattice("d3").apply(vt)
    assert torch.equal(plx.filter(vt, xt, ct), want)
    assert torch.equal(ext.filter(vt, xt, ct), want)
    h = ext.LatticeHandle(0)
    h.build(xt, ct)
    assert torch.equal(h.apply(vt), want) and h.apply(vt.float()).dtype == torch.float32
    with pytest.raises(TypeError):
        plx.filter(vt, xt.float(), ct)
    with pytest.raises(RuntimeError, match="float32"):
        ext.filter(vt, xt.float(), ct)
    # the operator classes: a double model's kernel matrix times a double right-hand side, square and rectangular
    try:
        k = plx.RBFLattice(order=1, ard_num_dims=3).double().cuda()
        with torch.no_grad():
            sq = k(xt, xt).matmul(vt)
            assert sq.dtype == torch.float64 and sq.shape == (n, 3)
            ell = k.lengthscale.detach()
            ref = Lattice64((xt / ell).float().cpu().numpy(), k.dkernel_fn.get_coeffs().numpy())
            assert rel_l2(sq.cpu().numpy(), ref.apply_staged(v)) <= 1e-12
            xs = cuda(np.random.default_rng(2).standard_normal((500, 3)), np.float64)
            rect = k(xs, xt).matmul(vt)
            assert rect.dtype == torch.float64 and rect.shape == (500, 3)
            big = Lattice64(torch.cat([xt / ell, xs / ell]).float().cpu().numpy(), k.dkernel_fn.get_coeffs().numpy())
            padded = np.concatenate([v, np.zeros((500, 3))])
            assert rel_l2(rect.cpu().numpy(), big.apply_staged(padded)[n:]) <= 1e-12
            builds = plx.lattice_cache().misses
            assert torch.equal(k(xt, xt).matmul(vt), sq)                  # the lattice cache serves double positions too
            assert plx.lattice_cache().misses == builds
    finally:
        plx.lattice_cache().clear()


def family_report():
    lines = ["native fp64 against Lattice64, worst per family (entry ratio / its bar k 2^-52, rel-L2 / its bar, entry ratio):"]
    for fam, (a, b, e, c) in sorted(WORST.items()):
        lines.append(f"  {fam[0]} | {fam[1]} | {fam[2]}: {a:.3f} {b:.3f} {e:.2e} ({c} cases)")
    lines.append("fp32 against native fp64, worst per fp32 family (entry ratio, rel-L2):")
    for fam, (e, r, c) in sorted(WORST32.items()):
        lines.append(f"  {' | '.join(fam)}: {e:.2e} {r:.2e} ({c} cases)")
    return "\n".join(lines)


def test_every_family_was_reached():
    """Every kernel name plx_f64.hip can report ran in this module (run as a whole), each inside the family expect() names."""
    import os
    import re
    print(family_report())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "simplex_gp_amd", "csrc", "plx_f64.hip")).read()
    literals = set()
    for stmt in re.finditer(r"\bkn_f64_(?:splat|blur|slice)\s*=([^;]*);", text):
        literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    assert literals == {s for fam in FAMILIES for s in fam}, literals
    assert set(WORST) == set(FAMILIES), sorted(WORST)
    assert REACHED == literals, sorted(literals - REACHED)
