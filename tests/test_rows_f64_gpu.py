"""The float64 rectangular product K[out rows, src rows] v (plx_splat_rows_f64 / plx_slice_rows_f64 / plx_apply_rows_f64,
simplex_gp_amd/csrc/plx_rows_f64.hip) on the GPU.

Per case, in this order:
  1. determinism and the steady state: three calls bit-equal, plx_device_bytes does not move between the second and the
     third, Lattice.rows_f64_kernels() names the family the width implies (chunks of two doubles: vd = 1, 1..64, wider);
  2. the bit contract: torch.equal to rows [out_begin, out_begin + out_count) of the float64 Lattice.apply of the right-hand
     side padded with zeros outside the source rows (the full range on both ends: to Lattice.apply itself);
  3. tests/lattice64.Lattice64 on the padded right-hand side with the DERIVED bar of tests/test_f64_gpu.py: entry ratio
     <= k 2^-52 of T = terms64(padded), k = depth(lat) -- Lmax taken from the exported full PLX_ARRAY_ROW_PTR, an upper bound
     for the rows of any range --, rel-L2 <= k 2^-52 ||T|| / ||want||, and exactly 0 where T_i = 0 (entry_ratio is inf
     otherwise);
  4. the staged form: splat_rows + blur + slice_rows in double is torch.equal to apply_rows.
The worst ratios against their bars per family are printed at the end of the module (pytest -s); DESIGN.md section 15 lists
them.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd._native import PlxError
from tests import test_f64_gpu as sq64
from tests.lattice64 import Lattice64, cloud, entry_ratio, rel_l2
from tests.test_f64_gpu import U2, cuda, depth, gauss_taps, placed
from tests.test_rows_fp64 import RANGES, ranges

pytestmark = pytest.mark.gpu

PLX_ERR_INVALID, PLX_ERR_STATE = 1, 5
F64 = torch.float64

V1 = ("rows64_splat_v1_kernel", "rows64_slice_v1_kernel")
CHUNK = ("rows64_splat_chunk_kernel", "rows64_slice_chunk_kernel")
WIDE = ("rows64_splat_wide_kernel", "rows64_slice_wide_kernel")


def expect(vd):
    """The family plx_rows_f64.hip picks: by the row width alone (chunks of two doubles)."""
    nch = (vd + 1) // 2
    return V1 if vd == 1 else CHUNK if nch <= 64 else WIDE


# name -> (cloud, n, d, order): the smallest that still reach every code path
LATTICES = {
    "d1": ("gauss1", 3001, 1, 1),
    "d3": ("gauss1", 3000, 3, 2),
    "d8": ("gauss1", 3000, 8, 3),
    "d18": ("gauss1", 1500, 18, 1),          # sparse: m = n (d + 1), every corner its own vertex
    "coarse": ("gauss0.3", 4000, 3, 1),      # coarse: hundreds of corners per vertex row
    "d24": ("gauss1", 600, 24, 1),           # d + 1 > 20: the slices' run-time form; its own two cases, not the rotation
}
# 2: one chunk; 128: 64 chunks, the last of the chunk family; 129: the first of the wide family; odd: the guarded tail
VDS = (1, 2, 3, 11, 12, 128, 129, 520)


def _cases():
    out = []
    for i, lname in enumerate(l for l in LATTICES if l != "d24"):
        for j, vd in enumerate(VDS):
            if (i + j) % 4 == 3:                            # two widths per lattice left out, rotating: every width on >= 3 lattices
                continue
            out.append((lname, vd, RANGES[(2 * i + j) % len(RANGES)], (i + j) % 2 == 0))
    for j, vd in enumerate((1, 11, 129)):                   # every range at one lattice, a width of each family
        for k, rname in enumerate(RANGES):
            if not any(c[:3] == ("d8", vd, rname) for c in out):
                out.append(("d8", vd, rname, (j + k) % 2 == 1))
    out += [("d24", 1, "overlap", True), ("d24", 12, "overlap", False)]
    return out


CASES = _cases()
assert len(CASES) <= 60
_OPS, _LATS = {}, {}


def operator(lname):
    """(x, Lattice64, taps) of a named lattice, built once (the ones tests/test_f64_gpu.py builds too are shared with it)."""
    if lname not in _OPS:
        if sq64.LATTICES.get(lname) == LATTICES[lname]:
            _OPS[lname] = sq64.operator(lname)
        else:
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


WORST = {}        # family -> [entry ratio / (k 2^-52), rel-L2 / its bar, entry ratio, cases]
REACHED = set()


def family_of(lat):
    k = lat.rows_f64_kernels()
    return ("+".join(k["splat"]), "+".join(k["slice"]))


def check(lat, l64, vd, src_rng, out_rng, aligned, seed, label):
    """All per-case assertions; returns the output rows."""
    n = l64.n
    (sb, sc), (ob, oc) = src_rng, out_rng
    v = np.random.default_rng(seed).standard_normal((sc, vd))
    padded = np.zeros((n, vd))
    padded[sb:sb + sc] = v
    src = placed(sc, vd, aligned, cuda(v, np.float64))
    # 1. determinism and the steady state
    got = [lat.apply_rows(src, sb, ob, oc, out=placed(oc, vd, aligned)).clone()]
    got.append(lat.apply_rows(src, sb, ob, oc, out=placed(oc, vd, aligned)).clone())
    bytes2 = lat.device_bytes
    got.append(lat.apply_rows(src, sb, ob, oc, out=placed(oc, vd, aligned)).clone())
    assert lat.device_bytes == bytes2, (label, "a steady-state fp64 rows call moved plx_device_bytes")
    assert got[0].dtype == F64 and torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), (label, "not deterministic")
    fam = family_of(lat)
    assert fam == expect(vd), (label, fam)
    REACHED.update(fam)
    # 2. the bit contract
    square = lat.apply(cuda(padded, np.float64))[ob:ob + oc]
    assert torch.equal(got[0], square), (label, "differs from the rows of the padded float64 product",
                                         float((got[0] - square).abs().max()))
    # 3. Lattice64, the derived bar
    want, T = l64.apply_staged(padded)[ob:ob + oc], l64.terms64(padded)[ob:ob + oc]
    out = got[0].cpu().numpy()
    k = depth(lat)
    e, r = entry_ratio(out, want, T), rel_l2(out, want)
    rbar = k * U2 * float(np.linalg.norm(T)) / max(float(np.linalg.norm(want)), 1e-300)
    print(f"{label}: k = {k}  entry {e:.2e} (bar {k * U2:.2e})  rel-L2 {r:.2e} (bar {rbar:.2e})  {fam[0]} {fam[1]}")
    assert e <= k * U2, (label, "entry ratio", e, k * U2)
    assert r <= rbar, (label, "rel-L2", r, rbar)
    w = WORST.setdefault(fam, [0.0, 0.0, 0.0, 0])
    w[0], w[1], w[2], w[3] = max(w[0], e / (k * U2)), max(w[1], r / rbar if rbar > 0 else 0.0), max(w[2], e), w[3] + 1
    # 4. the staged form
    values = lat.splat_rows(src, sb)
    assert values.dtype == F64 and values.shape == (lat.m, plx.Lattice.values_stride(vd, F64))
    staged = lat.slice_rows(lat.blur(values, vd=vd), ob, oc, out=placed(oc, vd, aligned), vd=vd)
    assert torch.equal(staged, got[0]), (label, "splat_rows + blur + slice_rows differs from apply_rows")
    assert family_of(lat) == fam
    return got[0]


@pytest.mark.parametrize("lname,vd,rname,aligned", CASES,
                         ids=[f"{a}-vd{b}-{c}-{'al' if d else 'off'}" for a, b, c, d in CASES])
def test_rows_f64_product(lname, vd, rname, aligned):
    x, l64, _ = operator(lname)
    kind, n, d, order = LATTICES[lname]
    if lname == "d18":
        assert l64.m == n * (d + 1)                     # the sparse lattice the case is named for
    if lname == "coarse":
        assert l64.m * 100 < n * (d + 1)                # ... and the coarse one
    lat = gpu_lattice(lname)
    assert lat.m == l64.m and lat.d + 1 == d + 1
    src_rng, out_rng = ranges(rname, n)
    out = check(lat, l64, vd, src_rng, out_rng, aligned, seed=vd + 7, label=f"{lname} vd={vd} {rname}")
    if rname == "full":                                 # the full range on both ends is the float64 product
        v = np.random.default_rng(vd + 7).standard_normal((n, vd))
        assert torch.equal(out, lat.apply(cuda(v, np.float64)))


def test_two_clusters_far_apart_give_exact_zeros():
    """Sources in one cluster, outputs in another that no blur reaches: every output is exactly 0, in both directions."""
    from oracle import oracle
    n, d, taps = 4000, 3, gauss_taps(1)
    sf = oracle.scale_factors(d, taps)
    x = (np.random.default_rng(3).standard_normal((n, d)) * 0.5).astype(np.float32)
    x[n // 2:, 0] += np.float32(60.0 * d / float(sf[0]))
    l64 = Lattice64(x, taps)
    lat = plx.Lattice().build(cuda(x), taps)
    for vd, aligned in ((1, True), (11, False), (129, True)):
        src_rng, out_rng = (0, n // 2), (n // 2, n - n // 2)
        padded = np.zeros((n, vd))
        padded[:n // 2] = 1.0
        assert l64.terms64(padded)[n // 2:].max() == 0.0           # the case is what it claims to be
        out = check(lat, l64, vd, src_rng, out_rng, aligned, seed=vd, label=f"clusters vd={vd}")
        assert int(torch.count_nonzero(out)) == 0
        out = check(lat, l64, vd, out_rng, src_rng, aligned, seed=vd + 1, label=f"clusters vd={vd} transposed")
        assert int(torch.count_nonzero(out)) == 0
    lat.close()


def test_range_tables_are_shared_between_the_precisions():
    x, l64, taps = operator("d8")
    n, vd = l64.n, 12
    k = int(0.8 * n)
    a, b = (0, k), (k, n - k)
    rng = np.random.default_rng(1)
    v, full = rng.standard_normal((k, vd)), rng.standard_normal((n, vd))
    V64, V32 = cuda(v, np.float64), cuda(v)
    # fp32 builds the tables of the pair, an fp64 product of the width the workspace: the first fp64 rows call finds both
    lat = plx.Lattice().build(cuda(x), taps)
    lat.apply_rows(V32, a[0], b[0], b[1])
    lat.apply(cuda(full, np.float64))
    before = lat.device_bytes
    got64 = lat.apply_rows(V64, a[0], b[0], b[1]).clone()
    assert lat.device_bytes == before, "the first fp64 rows call of a range fp32 had built moved plx_device_bytes"
    assert family_of(lat) == CHUNK
    lat.close()
    # the reverse: fp64 builds the tables, an fp32 product of the width the fp32 workspace
    lat = plx.Lattice().build(cuda(x), taps)
    assert torch.equal(lat.apply_rows(V64, a[0], b[0], b[1]), got64)
    lat.apply(cuda(full))
    before = lat.device_bytes
    got32 = lat.apply_rows(V32, a[0], b[0], b[1]).clone()
    assert lat.device_bytes == before, "the first fp32 rows call of a range fp64 had built moved plx_device_bytes"
    fresh = plx.Lattice().build(cuda(x), taps)
    assert torch.equal(got32, fresh.apply_rows(V32, a[0], b[0], b[1]))   # tables made by fp64 calls: the fresh lattice's bits
    fresh.close()
    # more ranges than the lattice keeps, in both precisions: the tables are rebuilt, the numbers stay
    for j in range(6):
        (lat.apply_rows(V64[:100 + j], j, 200, 50) if j % 2 else lat.apply_rows(V32[:100 + j], j, 200, 50))
    assert torch.equal(lat.apply_rows(V64, a[0], b[0], b[1]), got64)
    assert torch.equal(lat.apply_rows(V32, a[0], b[0], b[1]), got32)
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
    l3 = Lattice64(x3, taps)
    third = check(lat, l3, 11, src_rng, out_rng, True, seed=5, label="rebuild: warm, re-scaled")
    assert not torch.equal(second, third)
    check(lat, l3, 1, out_rng, src_rng, False, seed=6, label="rebuild: warm, transposed, vd=1")
    lat.close()


def test_refusals_on_a_real_lattice():
    lib = nv.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(1 << 15, dtype=F64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    torch.cuda.synchronize()

    def calls(h, sb, sc, ob, oc, vd=1):
        return (lib.plx_splat_rows_f64(h, p, sb, sc, vd, p, stream), lib.plx_slice_rows_f64(h, p, vd, ob, oc, p, stream),
                lib.plx_apply_rows_f64(h, p, sb, sc, vd, p, ob, oc, stream))

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
    assert calls(lat._h, -1, 4, -1, 4) == (1, 1, 1)                                                 # a negative begin
    assert calls(lat._h, 0, 2001, 0, 2001) == (1, 1, 1)
    assert calls(lat._h, 0, 4, 4, 4, vd=0) == (1, 1, 1)
    assert lib.plx_apply_rows_f64(lat._h, p, 0, 4, 1, p, 1999, 2, stream) == 1                      # only the output range is off
    assert b"plx_apply_rows_f64 (output rows)" in lib.plx_last_error()
    off8 = ctypes.c_void_p(buf.data_ptr() + 8)
    assert lib.plx_splat_rows_f64(lat._h, p, 0, 4, 3, off8, stream) == 1                            # values misaligned by 8 bytes
    assert b"16-byte" in lib.plx_last_error() and b"plx_splat_rows_f64" in lib.plx_last_error()
    assert lib.plx_slice_rows_f64(lat._h, off8, 3, 0, 4, p, stream) == 1 and b"16-byte" in lib.plx_last_error()
    assert lib.plx_apply_rows_f64(lat._h, ctypes.c_void_p(buf.data_ptr() + 4), 0, 4, 1, p, 4, 4, stream) == 1
    assert b"8-byte" in lib.plx_last_error()
    with pytest.raises(TypeError, match="float32 or float64"):
        lat.apply_rows(torch.zeros(4, 2, dtype=torch.float16, device="cuda"), 0, 4, 4)
    with pytest.raises(TypeError, match="like src"):
        lat.apply_rows(buf[:8].view(4, 2), 0, 4, 4, out=torch.zeros(4, 2, device="cuda"))
    lat.build(x, gauss_taps(1), shard=(0, 2))
    assert calls(lat._h, 0, 4, 4, 4) == (5, 5, 5) and b"sharded" in lib.plx_last_error()
    nv.check(lib.plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        g = torch.Generator().manual_seed(2008)
        ref = (torch.randn(2000, 8, generator=g) / 0.5).contiguous().cuda()
        lat.build(ref, np.array([0.34608543, 1.0, 0.34608543], np.float32))
        assert lat.reference_growth_info()["replayed"]
        assert calls(lat._h, 0, 4, 4, 4) == (5, 5, 5) and b"reference_growth" in lib.plx_last_error()
    finally:
        nv.check(lib.plx_tune(b"reference_growth", 0), "plx_tune")
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all())                                # none of the refused calls launched anything
    lat.build(x, gauss_taps(1))
    assert calls(lat._h, 0, 4, 4, 4) == (0, 0, 0)
    lat.close()


def test_capture():
    """One stream, no parallel branches: under capture a call that would build a range table (or grow the workspace) is
    PLX_ERR_STATE and the stream survives; a steady-state call captures and replays to the same bits."""
    rng = np.random.default_rng(3)
    n, d, vd = 20000, 4, 4
    k = int(0.8 * n)
    lat = plx.Lattice().build(cuda(rng.standard_normal((n, d))), gauss_taps(1))
    v = cuda(rng.standard_normal((k, vd)), np.float64)
    out = torch.empty((n - k, vd), dtype=F64, device="cuda")
    lat.apply(torch.zeros((n, vd), dtype=F64, device="cuda"))       # the float64 workspace of this width exists ...
    before = lat.device_bytes
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(PlxError, match="captured") as err:          # ... the tables of the range do not
        with torch.cuda.graph(graph, stream=s):
            lat.apply_rows(v, 0, k, n - k, out=out)
    assert err.value.code == PLX_ERR_STATE and lat.device_bytes == before
    del graph
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        eager = lat.apply_rows(v, 0, k, n - k, out=out).clone()
        first = lat.device_bytes
        assert first > before
        lat.apply_rows(v, 0, k, n - k, out=out)
        assert lat.device_bytes == first
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        out.zero_()
        with torch.cuda.graph(graph, stream=s):
            lat.apply_rows(v, 0, k, n - k, out=out)
        graph.replay()
        s.synchronize()
        assert torch.equal(out, eager)
        v2 = cuda(rng.standard_normal((k, vd)), np.float64)
        want2 = lat.apply_rows(v2, 0, k, n - k).clone()
        v.copy_(v2)
        graph.replay()
        s.synchronize()
        assert torch.equal(out, want2) and lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


@pytest.fixture()
def every_width():
    """The operator-level test wants the native route at its own (narrow) width: lift the shape gate for it."""
    keep = plx.RectangularLazyLattice.native_min_columns
    plx.RectangularLazyLattice.native_min_columns = 1
    yield
    plx.RectangularLazyLattice.native_min_columns = keep


def test_operator_level(every_width):
    """k(x*, x) @ V in double natively and padded: the same values; one lattice for the operator and its transpose; autograd
    in V; a gradient for the positions keeps the padded path."""
    torch.manual_seed(0)
    k = plx.RBFLattice(order=1, ard_num_dims=3).double().cuda()
    for prm in k.parameters():
        prm.requires_grad_(False)                                   # positions without a gradient: the native route
    n, ns, vd = 3000, 500, 4
    x, xs = torch.randn(n, 3, dtype=F64, device="cuda"), torch.randn(ns, 3, dtype=F64, device="cuda")
    V, G = torch.randn(n, vd, dtype=F64, device="cuda"), torch.randn(ns, vd, dtype=F64, device="cuda")
    cache = plx.lattice_cache()
    cache.clear()
    calls = []
    orig = plx.Lattice.apply_rows
    plx.Lattice.apply_rows = lambda self, *a, **kw: (calls.append(a[0].dtype), orig(self, *a, **kw))[1]
    keep = plx.RectangularLazyLattice.native_rows_f64
    try:
        plx.RectangularLazyLattice.native_rows_f64 = True
        assert plx.LatticeFilterGeneral.method is None and plx.RectangularLazyLattice.native_rows
        R = k(xs, x)
        m0 = cache.misses
        got = R.matmul(V)
        got_t = R.t().matmul(G)
        assert got.dtype == F64 and got_t.dtype == F64 and got.shape == (ns, vd) and got_t.shape == (n, vd)
        assert cache.misses == m0 + 1                               # ONE build: the transpose works on the same lattice
        assert calls == [F64, F64]
        lat = cache.get(R._stacked_points(), k.dkernel_fn.get_coeffs())
        assert cache.misses == m0 + 1 and family_of(lat) == CHUNK
        Vg = V.clone().requires_grad_()
        R.matmul(Vg).backward(G)
        assert cache.misses == m0 + 1 and len(calls) == 4
        assert Vg.grad.dtype == F64 and torch.equal(Vg.grad, got_t)
        # the padded path, the switch off: the same values
        plx.RectangularLazyLattice.native_rows_f64 = False
        del calls[:]
        R2 = k(xs, x)
        pad, pad_t = R2.matmul(V), R2.t().matmul(G)
        assert not calls
        assert torch.equal(got, pad), float((got - pad).abs().max())
        assert torch.equal(got_t, pad_t), float((got_t - pad_t).abs().max())
        # a gradient for the positions: the padded path runs, whatever the switch says
        grads = {}
        for on in (True, False):
            plx.RectangularLazyLattice.native_rows_f64 = on
            xg = xs.clone().requires_grad_()
            (k(xg, x).matmul(V) * G).sum().backward()
            grads[on] = xg.grad.clone()
        assert not calls and torch.equal(grads[True], grads[False]) and float(grads[True].abs().sum()) > 0
    finally:
        plx.Lattice.apply_rows = orig
        plx.RectangularLazyLattice.native_rows_f64 = keep
        cache.clear()


def test_every_rows_f64_family_was_reached():
    """The names Rows<double> (plx_rows_f64.hip) can report in kn_rows64_splat / kn_rows64_slice are exactly the six names,
    and all six ran above; the worst ratios against their bars per family."""
    src = open(os.path.join(os.path.dirname(nv.LIB_PATH), "csrc", "plx_rows_f64.hip")).read()
    block = re.search(r"struct Rows<double>\s*\{(.*?)\n\};", src, re.S).group(1)
    literals = set()
    for stmt in re.finditer(r"\bk(?:Splat|Slice)(?:V1|Chunk|Wide)\s*=([^;]*);", block):
        literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    assert literals == set(V1 + CHUNK + WIDE), literals
    print("\nfp64 rows kernels against Lattice64: worst entry ratio / its bar k 2^-52, rel-L2 / its bar, entry ratio (cases)")
    for fam, (a, b, e, c) in sorted(WORST.items()):
        print(f"  {fam[0]:28s} {fam[1]:28s} {a:.3f} {b:.3f} {e:.2e} ({c})")
    assert REACHED == literals, sorted(literals - REACHED)
    for lat in _LATS.values():
        lat.close()
    _LATS.clear()
