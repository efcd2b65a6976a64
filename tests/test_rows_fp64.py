"""The rectangular product K[out rows, src rows] v (plx_splat_rows / plx_slice_rows / plx_apply_rows) against float64.

The yardstick is tests/lattice64.Lattice64 on the FULL point set -- the float64 operator the forward tests use, built from
the CPU oracle's structure -- applied to the right-hand side padded with zeros outside the source rows, the output rows
cut afterwards.  Every case names the rows kernels it expects (plx_rows.hip: one family per stage for vd = 1, for rows of
1..64 chunks of 16 bytes, and for wider rows) and asserts that Lattice.rows_kernels() reports them;
test_every_rows_family_was_reached checks that every literal the source can report ran.

Per case, in this order: determinism (three calls bit-equal) and the steady state (plx_device_bytes does not move between
the second and the third call), the float64 bars, the padded square product on the same lattice, and the stage form
(splat_rows + blur + slice_rows bit-equal to apply_rows).

Bars, in float64: entry ratio max_i |got - want|_i / T_i with T = terms64 of the padded right-hand side (T_i = 0: got_i
must be exactly 0) and rel-L2.  Starting bars: 1e-5 each, where tests/test_forward_fp64.py started; the worst of both per
family is printed at the end of the module (pytest -s) and DESIGN.md section 13 lists them.  Measured worst over the three
families: entry 3.3e-7 of T, rel-L2 2.9e-6 (the coarse lattice at vd = 1: a vertex row there is one thread's sum of
thousands of terms, carried in order).  ENTRY is tightened to 4x its measured worst; 4x the measured rel-L2 (1.15e-5) lies
above the starting bar, so REL stays at the starting 1e-5.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from tests.lattice64 import Lattice64, cloud, entry_ratio, rel_l2
from tests.test_forward_fp64 import REL as SQUARE_REL

pytestmark = pytest.mark.gpu


@pytest.fixture()
def every_width():
    """The operator-level tests want the native route at their own (narrow) widths: lift the shape gate for them."""
    keep = plx.RectangularLazyLattice.native_min_columns
    plx.RectangularLazyLattice.native_min_columns = 1
    yield
    plx.RectangularLazyLattice.native_min_columns = keep

ENTRY = 1.4e-6    # per-entry error / size of its terms
REL = 1e-5        # rel-L2 of the output rows

V1 = ("rows_splat_v1_kernel", "rows_slice_v1_kernel")
CHUNK = ("rows_splat_chunk_kernel", "rows_slice_chunk_kernel")
WIDE = ("rows_splat_wide_kernel", "rows_slice_wide_kernel")


def expect(vd):
    """The family plx_rows.hip picks: by the row width alone."""
    nch = (vd + 3) // 4
    return V1 if vd == 1 else CHUNK if nch <= 64 else WIDE


def gauss_taps(order):
    half = np.exp(-0.5 * (np.arange(1, order + 1) * 0.7) ** 2)
    return np.concatenate([half[::-1], [1.0], half]).astype(np.float32)


# name -> (cloud, n, d, order)
LATTICES = {
    "d1": ("gauss1", 5000, 1, 1),          # a handful of vertices
    "d3": ("gauss1", 6000, 3, 2),
    "d8": ("gauss1", 6000, 8, 3),
    "d18": ("gauss1", 3000, 18, 1),        # sparse: m = n (d + 1), every corner its own vertex
    "coarse": ("gauss0.3", 20000, 3, 1),   # coarse: thousands of corners per vertex row
    "d8o1": ("gauss3", 4000, 8, 1),
    "d24": ("gauss1", 600, 24, 1),         # d + 1 > 20: the chunk slice's run-time form; its own two cases, not the grid
}
VDS = (1, 3, 4, 11, 12, 101, 130, 512, 520)
RANGES = ("head0.8", "head0.8T", "head0.5", "head0.5T", "one", "oneT", "equal", "overlap", "full")


def ranges(name, n):
    """((src_begin, src_count), (out_begin, out_count))"""
    if name.startswith("head") or name.startswith("one"):
        k = 1 if name.startswith("one") else int(float(name[4:7]) * n)
        a, b = (0, k), (k, n - k)
        return (b, a) if name.endswith("T") else (a, b)
    if name == "equal":
        return (n // 4, n // 2), (n // 4, n // 2)
    if name == "overlap":
        return (0, int(0.6 * n)), (int(0.4 * n), n - int(0.4 * n))
    assert name == "full"
    return (0, n), (0, n)


def _cases():
    out = []
    for i, lname in enumerate(l for l in LATTICES if l != "d24"):
        for j, vd in enumerate(VDS):
            out.append((lname, vd, RANGES[(2 * i + j) % len(RANGES)], (i + j) % 2 == 0))
    for j, vd in enumerate((1, 11, 101)):                  # every range at one lattice, a width of each narrow kind
        for k, rname in enumerate(RANGES):
            case = ("d8", vd, rname, (j + k) % 2 == 1)
            if case not in out:
                out.append(case)
    out += [("d24", 1, "overlap", True), ("d24", 12, "overlap", False)]
    return out


CASES = _cases()

_OPS = {}
_LATS = {}


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


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def placed(rows, vd, aligned, fill=None):
    """A contiguous [rows, vd] CUDA tensor whose data pointer is 16-byte aligned, or that plus one float."""
    buf = torch.empty(rows * vd + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[(0 if aligned else 1):(0 if aligned else 1) + rows * vd].view(rows, vd)
    assert t.is_contiguous() and t.data_ptr() % 16 == (0 if aligned else 4)
    if fill is not None:
        t.copy_(fill)
    else:
        t.fill_(float("nan"))
    return t


WORST = {}        # family -> [entry ratio, rel-L2, cases]
REACHED = set()


def check(lat, l64, vd, src_rng, out_rng, aligned, seed, label):
    """All per-case assertions; returns the output rows."""
    n = l64.n
    (sb, sc), (ob, oc) = src_rng, out_rng
    v = np.random.default_rng(seed).standard_normal((sc, vd)).astype(np.float32)
    padded = np.zeros((n, vd), np.float32)
    padded[sb:sb + sc] = v
    src = placed(sc, vd, aligned, cuda(v))
    # determinism and the steady state
    got = [lat.apply_rows(src, sb, ob, oc, out=placed(oc, vd, aligned)).clone()]
    got.append(lat.apply_rows(src, sb, ob, oc, out=placed(oc, vd, aligned)).clone())
    bytes2 = lat.device_bytes
    got.append(lat.apply_rows(src, sb, ob, oc, out=placed(oc, vd, aligned)).clone())
    assert lat.device_bytes == bytes2, (label, "a steady-state rows call moved plx_device_bytes")
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), (label, "not deterministic")
    k = lat.rows_kernels()
    fam = ("+".join(k["splat"]), "+".join(k["slice"]))
    assert fam == expect(vd), (label, fam)
    REACHED.update(fam)
    # float64
    want = l64.apply_staged(padded)[ob:ob + oc]
    T = l64.terms64(padded)[ob:ob + oc]
    out = got[0].cpu().numpy()
    e, r = entry_ratio(out, want, T), rel_l2(out, want)
    w = WORST.setdefault(fam, [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], e), max(w[1], r), w[2] + 1
    print(f"{label}: entry {e:.2e} rel-L2 {r:.2e} {fam[0]} {fam[1]}")
    assert e <= ENTRY and r <= REL, (label, e, r)
    # the padded square product on the same lattice
    square = lat.apply(cuda(padded))[ob:ob + oc].cpu().numpy()
    rs = rel_l2(out, square)
    assert rs <= REL + SQUARE_REL, (label, "against the padded square product", rs)
    # the stage form
    values = lat.splat_rows(src, sb)
    staged = lat.slice_rows(lat.blur(values, vd=vd), ob, oc, out=placed(oc, vd, aligned), vd=vd)
    assert torch.equal(staged, got[0]), (label, "splat_rows + blur + slice_rows differs from apply_rows")
    return got[0]


@pytest.mark.parametrize("lname,vd,rname,aligned", CASES,
                         ids=[f"{a}-vd{b}-{c}-{'al' if d else 'off'}" for a, b, c, d in CASES])
def test_rows_product_against_fp64(lname, vd, rname, aligned):
    x, l64, _ = operator(lname)
    kind, n, d, order = LATTICES[lname]
    if lname == "d18":
        assert l64.m == n * (d + 1)                     # the sparse lattice the case is named for
    if lname == "coarse":
        assert l64.m * 100 < n * (d + 1)                # ... and the coarse one
    lat = gpu_lattice(lname)
    assert lat.m == l64.m
    src_rng, out_rng = ranges(rname, n)
    out = check(lat, l64, vd, src_rng, out_rng, aligned, seed=vd + 7, label=f"{lname} vd={vd} {rname}")
    if rname == "full":                                 # the full range on both ends is plx_apply
        v = np.random.default_rng(vd + 7).standard_normal((n, vd)).astype(np.float32)
        assert rel_l2(out.cpu().numpy(), lat.apply(cuda(v)).cpu().numpy()) <= REL + SQUARE_REL


def test_two_clusters_far_apart_give_exact_zeros():
    """Sources in one cluster, outputs in another that no blur reaches: every output is exactly 0."""
    from oracle import oracle
    n, d, taps = 4000, 3, gauss_taps(1)
    sf = oracle.scale_factors(d, taps)
    x = (np.random.default_rng(3).standard_normal((n, d)) * 0.5).astype(np.float32)
    x[n // 2:, 0] += np.float32(60.0 * d / float(sf[0]))
    l64 = Lattice64(x, taps)
    lat = plx.Lattice().build(cuda(x), taps)
    for vd, aligned in ((1, True), (11, False), (101, True), (520, False)):
        src_rng, out_rng = (0, n // 2), (n // 2, n - n // 2)
        padded = np.zeros((n, vd), np.float32)
        padded[:n // 2] = 1.0
        assert l64.terms64(padded)[n // 2:].max() == 0.0           # the case is what it claims to be
        out = check(lat, l64, vd, src_rng, out_rng, aligned, seed=vd, label=f"clusters vd={vd}")
        assert int(torch.count_nonzero(out)) == 0
        out = check(lat, l64, vd, out_rng, src_rng, aligned, seed=vd + 1, label=f"clusters vd={vd} transposed")
        assert int(torch.count_nonzero(out)) == 0
    lat.close()


def test_cached_ranges_alternate_without_allocating():
    """product, transpose, product, transpose: the two cached ranges alternate, plx_device_bytes stays put, numbers too."""
    x, l64, taps = operator("d8o1")
    n = l64.n
    lat = plx.Lattice().build(cuda(x), taps)
    k = int(0.8 * n)
    a, b = (0, k), (k, n - k)
    V, G = cuda(np.random.default_rng(1).standard_normal((k, 12))), cuda(np.random.default_rng(2).standard_normal((n - k, 12)))
    outs, sizes = [], []
    for _ in range(3):
        outs.append((lat.apply_rows(V, a[0], b[0], b[1]).clone(), lat.apply_rows(G, b[0], a[0], a[1]).clone()))
        sizes.append(lat.device_bytes)
    assert sizes[1] == sizes[2], sizes
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    # more ranges than the lattice keeps: the tables are rebuilt, the numbers stay
    for j in range(6):
        lat.apply_rows(V[:100 + j], j, 200, 50)
    assert torch.equal(lat.apply_rows(V, a[0], b[0], b[1]), outs[0][0])
    assert torch.equal(lat.apply_rows(G, b[0], a[0], a[1]), outs[0][1])
    lat.close()


def test_rebuild_invalidates_the_cached_tables():
    """After build on new positions, and after the warm in-place rebuild, the same ranges give the NEW lattice's numbers."""
    kind, n, d, order = LATTICES["d3"]
    taps = gauss_taps(order)
    x1 = cloud(kind, n, d, seed=21, coeffs=taps)
    x2 = cloud(kind, n, d, seed=22, coeffs=taps)
    x3 = (x2 * np.float32(0.9)).astype(np.float32)
    lat = plx.Lattice().build(cuda(x1), taps)
    src_rng, out_rng = ranges("head0.8", n)
    first = check(lat, Lattice64(x1, taps), 11, src_rng, out_rng, True, seed=5, label="rebuild: first build")
    lat.build(cuda(x2), taps)
    second = check(lat, Lattice64(x2, taps), 11, src_rng, out_rng, True, seed=5, label="rebuild: new positions")
    assert not torch.equal(first, second)
    lat.build(cuda(x3), taps, reuse_order=True)
    assert lat.order_age == 1                                       # the warm rebuild did run
    third = check(lat, Lattice64(x3, taps), 11, src_rng, out_rng, True, seed=5, label="rebuild: warm, re-scaled")
    assert not torch.equal(second, third)
    check(lat, Lattice64(x3, taps), 1, out_rng, src_rng, True, seed=6, label="rebuild: warm, transposed, vd=1")
    lat.close()


def test_errors_on_a_real_lattice():
    lib = nv.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(1 << 16, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    torch.cuda.synchronize()

    def calls(h, sb, sc, ob, oc, vd=1):
        return (lib.plx_splat_rows(h, p, sb, sc, vd, p, stream), lib.plx_slice_rows(h, p, vd, ob, oc, p, stream),
                lib.plx_apply_rows(h, p, sb, sc, vd, p, ob, oc, stream))

    lat = plx.Lattice()
    x = cuda(cloud("gauss1", 2000, 3, seed=1))
    lat.build(x, gauss_taps(1))
    assert calls(lat._h, 0, 4, 4, 4) == (0, 0, 0)                  # (the same arguments on a lattice that serves them)
    torch.cuda.synchronize()
    buf.fill_(1.0)                                                 # every call from here on is refused: nothing may write
    fresh = plx.Lattice()
    assert calls(fresh._h, 0, 4, 4, 4) == (5, 5, 5) and b"not built" in lib.plx_last_error()
    fresh.close()
    assert calls(lat._h, 1990, 11, 1990, 11) == (1, 1, 1) and b"range" in lib.plx_last_error()      # past n
    assert calls(lat._h, 0, 0, 0, 0) == (1, 1, 1)                                                   # count 0
    assert calls(lat._h, -1, 4, -1, 4) == (1, 1, 1)
    assert calls(lat._h, 0, 2001, 0, 2001) == (1, 1, 1)
    assert calls(lat._h, 0, 4, 4, 4, vd=0) == (1, 1, 1)
    assert lib.plx_apply_rows(lat._h, p, 0, 4, 1, p, 1999, 2, stream) == 1                          # only the output range is off
    assert lib.plx_splat_rows(lat._h, p, 0, 4, 3, ctypes.c_void_p(buf.data_ptr() + 4), stream) == 1
    assert b"aligned" in lib.plx_last_error()
    lat.build(x, gauss_taps(1), shard=(0, 2))
    assert calls(lat._h, 0, 4, 4, 4) == (5, 5, 5) and b"sharded" in lib.plx_last_error()
    assert not lat.accepts_rows()
    nv.check(lib.plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        g = torch.Generator().manual_seed(2008)
        ref = (torch.randn(2000, 8, generator=g) / 0.5).contiguous().cuda()
        lat.build(ref, np.array([0.34608543, 1.0, 0.34608543], np.float32))
        assert lat.reference_growth_info()["replayed"]
        assert calls(lat._h, 0, 4, 4, 4) == (5, 5, 5) and b"reference_growth" in lib.plx_last_error()
        assert not lat.accepts_rows()
    finally:
        nv.check(lib.plx_tune(b"reference_growth", 0), "plx_tune")
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all())                                # none of the refused calls launched anything
    lat.build(x, gauss_taps(1))
    assert lat.accepts_rows() and calls(lat._h, 0, 4, 4, 4) == (0, 0, 0)
    lat.close()


def test_operator_level(every_width):
    """k(x*, x) @ V natively and padded; one lattice for the operator and its transpose; autograd in V."""
    from simplex_gp_amd import lattice_kernel as lk
    torch.manual_seed(0)
    k = plx.RBFLattice(order=1, ard_num_dims=3).cuda()
    for prm in k.parameters():
        prm.requires_grad_(False)                                   # positions without a gradient: the native route
    n, ns, vd = 5000, 700, 4
    x, xs = torch.randn(n, 3, device="cuda"), torch.randn(ns, 3, device="cuda")
    V, G = torch.randn(n, vd, device="cuda"), torch.randn(ns, vd, device="cuda")
    cache = plx.lattice_cache()
    cache.clear()
    assert plx.LatticeFilterGeneral.method is None and plx.RectangularLazyLattice.native_rows
    R = k(xs, x)
    m0 = cache.misses
    got = R.matmul(V)
    got_t = R.t().matmul(G)
    assert got.shape == (ns, vd) and got_t.shape == (n, vd)
    assert cache.misses == m0 + 1                                   # ONE build: the transpose works on the same lattice
    stacked = R._stacked_points()
    coeffs = k.dkernel_fn.get_coeffs()
    lat = cache.get(stacked, coeffs)
    assert cache.misses == m0 + 1 and lat.rows_kernels() == {"splat": [CHUNK[0]], "slice": [CHUNK[1]]}
    l64 = Lattice64(stacked.cpu().numpy(), coeffs.numpy())
    pv = np.concatenate([V.cpu().numpy(), np.zeros((ns, vd), np.float32)])
    pg = np.concatenate([np.zeros((n, vd), np.float32), G.cpu().numpy()])
    for name, out, padded, rows in (("product", got, pv, slice(n, n + ns)), ("transpose", got_t, pg, slice(0, n))):
        e = entry_ratio(out.cpu().numpy(), l64.apply_staged(padded)[rows], l64.terms64(padded)[rows])
        r = rel_l2(out.cpu().numpy(), l64.apply_staged(padded)[rows])
        print(f"operator {name}: entry {e:.2e} rel-L2 {r:.2e}")
        assert e <= ENTRY and r <= REL, (name, e, r)
    # autograd in the right-hand side
    Vg = V.clone().requires_grad_()
    R.matmul(Vg).backward(G)
    assert cache.misses == m0 + 1
    want = l64.apply_staged(pg)[:n]
    e, r = entry_ratio(Vg.grad.cpu().numpy(), want, l64.terms64(pg)[:n]), rel_l2(Vg.grad.cpu().numpy(), want)
    print(f"operator grad V: entry {e:.2e} rel-L2 {r:.2e}")
    assert e <= ENTRY and r <= REL and torch.equal(Vg.grad, got_t)
    # the padded path: same numbers within both float64 bars
    plx.RectangularLazyLattice.native_rows = False
    try:
        R2 = k(xs, x)
        pad, pad_t = R2.matmul(V), R2.t().matmul(G)
    finally:
        plx.RectangularLazyLattice.native_rows = True
    assert rel_l2(got.cpu().numpy(), pad.cpu().numpy()) <= REL + SQUARE_REL
    assert rel_l2(got_t.cpu().numpy(), pad_t.cpu().numpy()) <= REL + SQUARE_REL
    # a gradient for the positions: the padded path runs, whatever the switch says
    calls = []
    orig = plx.Lattice.apply_rows
    plx.Lattice.apply_rows = lambda self, *a, **kw: (calls.append(1), orig(self, *a, **kw))[1]
    grads = {}
    try:
        for on in (True, False):
            plx.RectangularLazyLattice.native_rows = on
            xg = xs.clone().requires_grad_()
            (k(xg, x).matmul(V) * G).sum().backward()
            grads[on] = xg.grad.clone()
    finally:
        plx.Lattice.apply_rows = orig
        plx.RectangularLazyLattice.native_rows = True
    assert not calls and torch.equal(grads[True], grads[False]) and float(grads[True].abs().sum()) > 0
    assert isinstance(lk.LatticeRowsProduct, type)
    cache.clear()


def test_shape_gate_keeps_narrow_products_on_the_padded_path():
    """Below native_min_columns the padded path runs (no rows call); from it on the native one."""
    k = plx.RBFLattice(order=1, ard_num_dims=2).cuda()
    x, xs = torch.randn(3000, 2, device="cuda"), torch.randn(400, 2, device="cuda")
    lo = plx.RectangularLazyLattice.native_min_columns
    calls = []
    orig = plx.Lattice.apply_rows
    plx.Lattice.apply_rows = lambda self, *a, **kw: (calls.append(1), orig(self, *a, **kw))[1]
    try:
        with torch.no_grad():
            R = k(xs, x)
            narrow = R.matmul(torch.randn(3000, lo - 1, device="cuda"))
            assert not calls and narrow.shape == (400, lo - 1)
            wide = R.matmul(torch.randn(3000, lo, device="cuda"))
            assert len(calls) == 1 and wide.shape == (400, lo)
    finally:
        plx.Lattice.apply_rows = orig
    plx.lattice_cache().clear()


def test_prediction_on_snelson(golden_dir, every_width):
    """training.predict with the native route and with the padded one: mean and variance within 1e-5 max(1, |value|)."""
    from simplex_gp_amd import solvers, training
    sn = np.loadtxt(os.path.join(golden_dir, "snelson.csv"), delimiter=",", skiprows=1).astype(np.float32)
    x, y = torch.from_numpy(sn[:, :1].copy()).cuda(), torch.from_numpy(sn[:, 1].copy()).cuda()
    xs = torch.linspace(-0.5, 6.5, 57, device="cuda").unsqueeze(-1)
    torch.manual_seed(0)
    model = solvers.LatticeGP(plx.RBFLattice(order=1)).cuda()
    res = {}
    for on in (True, False):
        plx.RectangularLazyLattice.native_rows = on
        try:
            plx.lattice_cache().clear()
            res[on] = training.predict(model, x, y, xs, cg_tol=1e-6, lanc_iter=50)
        finally:
            plx.RectangularLazyLattice.native_rows = True
    for name, a, b in (("mean", res[True][0], res[False][0]), ("variance", res[True][1], res[False][1])):
        gap = (a - b).abs() / b.abs().clamp_min(1.0)
        print(f"snelson {name}: worst gap {float(gap.max()):.2e} of max(1, |value|)")
        assert float(gap.max()) <= 1e-5, name
    plx.lattice_cache().clear()


def test_every_rows_family_was_reached():
    """Every name Rows<float> (plx_rows.hip) can report in kn_rows_splat / kn_rows_slice ran above; the worst bars per family."""
    src = open(os.path.join(os.path.dirname(nv.LIB_PATH), "csrc", "plx_rows.hip")).read()
    block = re.search(r"struct Rows<float>\s*\{(.*?)\n\};", src, re.S).group(1)
    literals = set()
    for stmt in re.finditer(r"\bk(?:Splat|Slice)(?:V1|Chunk|Wide)\s*=([^;]*);", block):
        literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    assert literals == set(V1 + CHUNK + WIDE), literals
    print("\nrows kernels against float64: worst entry ratio / rel-L2 per family (cases)")
    for fam, (e, r, c) in sorted(WORST.items()):
        print(f"  {fam[0]:26s} {fam[1]:26s} {e:.2e} {r:.2e} ({c})")
    assert literals <= REACHED, literals - REACHED
    for lat in _LATS.values():
        lat.close()
    _LATS.clear()
