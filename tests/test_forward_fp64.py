"""The forward lattice product K v = slice(blur(splat(v))) against float64 at every kernel family the dispatcher picks.

Each stage has several kernel families (plx_splat.hip, plx_first.hip, plx_block.hip, plx_blur.hip, plx_slice.hip,
plx_onehot.hip).  Which one runs depends on vd, the order, m, sparsity, row order, alignment and the plx_tune switches.
Every case here names the (splat, blur_axis, slice) family it expects, asserts that Lattice.stage_kernels() reports
exactly that, and compares the output with the float64 operator of tests/lattice64.py on the same duplicate-free
structure.  FAMILIES maps each family to the cases that reach it.  test_every_family_was_reached checks that all of them
ran.  tests/test_lattice64.py checks that FAMILIES names every kn_splat / kn_blur / kn_slice literal of the sources.

Bars, in float64, per entry and overall:
  * entry ratio  max_i |got - want|_i / T_i with T = lattice64.terms64(v), the size of the terms entry i sums (T_i = 0:
    got_i must be exactly 0);
  * rel-L2       ||got - want|| / ||want||.
The worst of both per family is printed at the end of the module (pytest -s).  DESIGN.md section 11 lists them.
"""
import contextlib

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from tests.lattice64 import Lattice64, cloud, entry_ratio, rel_l2

pytestmark = pytest.mark.gpu

# Starting bars 1e-5 of T and rel-L2 1e-5, tightened to 4x the measured worst over all 42 families:
# entry 4.4e-7 of T, rel-L2 4.0e-7, the column dots 4.3e-8 of sum |v| |out|.
ENTRY = 1.8e-6    # per-entry error / size of its terms
REL = 1.6e-6      # rel-L2 of the whole output
DOT = 1.8e-7      # apply_affine_dot: |dot - <v, out>| / sum |v| |out|

# ---- family names (the literals of the sources) ---------------------------------------------------------------------
SCAN = "splat_scan_kernel+splat_fixup_kernel"
SCAN_G1 = "gather_in_v1_kernel+splat_scan_kernel+splat_fixup_kernel"
SCAN_G = "gather_in_kernel+splat_scan_kernel+splat_fixup_kernel"
GROUP = "splat_group_kernel+splat_fixup_kernel"
GROUP_G = "gather_in_kernel+splat_group_kernel+splat_fixup_kernel"
WIDE = "splat_wide_kernel+splat_fixup_kernel"
WIDE_G = "gather_in_kernel+splat_wide_kernel+splat_fixup_kernel"
FIRST_SEQ = "splat_first_seq_kernel"
FIRST_SEQ_X = "splat_first_seq_kernel+splat_extras_kernel"
FIRST = "splat_first_kernel"
FIRST_X = "splat_first_kernel+splat_extras_kernel"
BLOCK = "splat_block_kernel+splat_combine_kernel"
SPLAT_ONEHOT = "splat_onehot_kernel"
SEED = "onehot_seed_kernel"
BACKWARD = "backward_pack_kernel+splat_wide_kernel+splat_fixup_kernel"

SMALL = "blur_small_kernel"
V1 = "blur_axis_v1_kernel"
COMPACT = "blur_axis_compact_kernel"
PAIR_V1 = "blur_pair_v1_kernel"
PAIR_V1_ODD = "blur_pair_v1_kernel+blur_axis_v1_kernel"
GENERAL = "blur_axis_kernel"
NARROW = "blur_axis_narrow_kernel"
PAIR_NARROW = "blur_pair_narrow_kernel"
PAIR_NARROW_ODD = "blur_pair_narrow_kernel+blur_axis_narrow_kernel"
MULTI = "blur_axis_multi_kernel"
ACTIVE = "blur_active_rows_kernel+blur_active_store_kernel"
OH_AXIS = "onehot_axis_kernel"
OH_PAIR = "onehot_pair_kernel"

SLICE_V1 = "slice_v1_kernel"
VEC = "slice_vec_kernel"
VEC_UNPERM = "slice_vec_kernel+unpermute_rows_kernel"
VEC_UNPERM_LDS = "slice_vec_kernel+unpermute_rows_lds_kernel"
SLICE_BLOCK = "slice_block_kernel"
SLICE_BLOCK_UNPERM = "slice_block_kernel+unpermute_kernel"
OH_SLICE = "onehot_slice_kernel"
CONTRACT = None                 # the fused backward's slice_contract kernels name no slice (test_backward_fp64 checks them)

# ---- switches -------------------------------------------------------------------------------------------------------
DEFAULTS = {"block_path": 1, "block_e": 0, "splat_first": 1, "splat_direct": 1, "splat_wide": 1, "splat_group": 1,
            "compact_nbr": 1, "blur_small": 1, "blur_vpt": 4, "blur_fuse": 1, "blur_fuse_vec": 1, "blur_multi": 1,
            "blur_narrow": 1, "blur_active": 1, "perm_rows": 1, "unpermute_gather": 1, "vertex_order": 1}   # plx_internal.h
# The module's baseline: the vd = 1 block / first-touch paths, the compacted neighbour table and the active-row blur
# are chosen per lattice from its sparsity; off by default here so that the expected family follows from the shape.
BASE = dict(DEFAULTS, block_path=0, splat_first=0, compact_nbr=0, blur_active=0)


def set_switches(sw):
    lib = nv.lib()
    for k, v in sw.items():
        nv.check(lib.plx_tune(k.encode(), int(v)), "plx_tune")


@pytest.fixture(scope="module", autouse=True)
def baseline_switches():
    set_switches(BASE)
    yield
    set_switches(DEFAULTS)


@contextlib.contextmanager
def tuned(**sw):
    """Process-wide switches for the builds (and one-shot filters) inside; back to BASE afterwards.  A lattice works
    under the snapshot taken when its build starts, so these hold for its MVMs too."""
    set_switches(sw)
    try:
        yield
    finally:
        set_switches({k: BASE[k] for k in sw})


def expect(vd, d, order=1, *, m=0, lattice_rows=False, aligned=True, single_use=False, compact=False, active=False,
           n=0, dot=False, **sw):
    """The family the dispatcher picks for this shape under BASE + `sw`, as plx_splat / plx_blur / plx_slice.hip decide.
    compact / active: whether the build chose the compacted table / the active-row lists (they depend on sparsity)."""
    t = dict(BASE, **sw)
    d1, nch = d + 1, (vd + 3) // 4
    if vd == 1:
        splat = SCAN if (lattice_rows or t["splat_direct"]) else SCAN_G1
    else:
        g = "" if (lattice_rows and vd % 4 == 0 and aligned) else "gather_in_kernel+"
        if t["splat_wide"] and (32 if t["splat_wide"] >= 2 else 17) <= nch <= 128:
            splat = g + WIDE
        elif t["splat_group"] and 2 <= nch <= 16:
            splat = g + GROUP
        else:
            splat = g + SCAN
    v1 = vd == 1 and 1 <= order <= 3 and t["blur_vpt"] in (2, 4)
    pair_vec = (vd > 1 and order == 1 and t["blur_fuse_vec"] and not single_use and t["blur_narrow"] and 2 <= nch <= 4
                and d1 >= 2)
    use_pairs = order == 1 and (t["blur_fuse"] == 2 or (t["blur_fuse"] == 1 and m <= 600000 and not single_use))
    if v1 and m <= 16384 and t["blur_small"]:
        blur = SMALL
    elif active:
        blur = ACTIVE
    elif pair_vec:
        blur = PAIR_NARROW_ODD if d1 & 1 else PAIR_NARROW
    elif v1 and order == 1 and use_pairs and not compact:
        blur = PAIR_V1_ODD if d1 & 1 else PAIR_V1
    elif v1:
        blur = COMPACT if compact else V1
    elif vd == 1:
        blur = GENERAL
    elif 1 <= order <= 3 and nch <= 4 and t["blur_narrow"]:
        blur = NARROW
    elif 1 <= order <= 3 and t["blur_multi"] and nch >= (32 if t["blur_multi"] >= 2 else 17):
        blur = MULTI
    else:
        blur = GENERAL
    if vd == 1:
        slc = SLICE_V1
    elif not lattice_rows and not dot and t["unpermute_gather"] and n * vd * 4 > (96 << 20):
        slc = VEC_UNPERM_LDS if (t["perm_rows"] and vd <= 48 and aligned) else VEC_UNPERM
    else:
        slc = VEC
    return (splat, blur, slc)


# ---- taps and cached float64 operators --------------------------------------------------------------------------------
def gauss_taps(order):
    half = np.exp(-0.5 * (np.arange(1, order + 1) * 0.7) ** 2)
    return np.concatenate([half[::-1], [1.0], half]).astype(np.float32)


def lopsided_taps(order):
    """Non-symmetric taps with a centre other than 1: a swapped tap index or an assumed unit centre shows."""
    half = np.exp(-0.5 * (np.arange(1, order + 1) * 0.7) ** 2)
    return np.concatenate([0.55 * half[::-1], [0.85], 1.15 * half]).astype(np.float32)


RBF1 = np.array([0.34608543, 1.0, 0.34608543], np.float32)
_L64 = {}


def operator(kind, n, d, taps, seed=0):
    """(x, Lattice64) for one cloud, built once for the whole module."""
    key = (kind, n, d, seed, taps.tobytes())
    if key not in _L64:
        x = cloud(kind, n, d, seed=seed, coeffs=taps)
        _L64[key] = (x, Lattice64(x, taps))
    return _L64[key]


def reference(l64, v):
    """(K64 v, terms64(v))."""
    want = l64.apply(v) if l64.n <= 3000 else l64.apply_staged(v)
    return want, l64.terms64(v)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def rhs(n, vd, seed):
    return np.random.default_rng(seed).standard_normal((n, vd)).astype(np.float32)


# ---- bookkeeping ------------------------------------------------------------------------------------------------------
WORST = {}        # family -> [entry ratio, rel-L2, cases]
REACHED = set()


def family_of(lat):
    k = lat.stage_kernels()
    return ("+".join(k["splat"]), "+".join(k["blur_axis"]), "+".join(k["slice"]))


def check(fam, got, want, T, what):
    """fam: the family that ran (already compared with the expectation)."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ratio = entry_ratio(got, want, T)
    rel = rel_l2(got, want) if np.linalg.norm(want) > 0 else 0.0
    row = WORST.setdefault(fam, [0.0, 0.0, 0])
    row[0], row[1], row[2] = max(row[0], ratio), max(row[1], rel), row[2] + 1
    REACHED.add(fam)
    assert ratio <= ENTRY, (what, fam, "entry ratio", ratio)
    assert rel <= REL, (what, fam, "rel-L2", rel)


def ran(lat, fam, what):
    assert fam in FAMILIES, ("expected a family FAMILIES does not list", fam)
    got = family_of(lat)
    if fam[2] is CONTRACT:
        got = got[:2] + (CONTRACT,)
    assert got == fam, (what, "expected", fam, "ran", got)
    return fam


def run_apply(lat, l64, v, fam, what, src=None):
    out = lat.apply(cuda(v) if src is None else src)
    want, T = reference(l64, v)
    check(ran(lat, fam, what), out, want, T, what)


@pytest.fixture(scope="module", autouse=True)
def family_report():
    yield
    if not WORST:
        return
    print(f"\nforward vs float64, worst per family (bars: entry {ENTRY:.1e} of T, rel-L2 {REL:.1e})")
    print(f"{'splat':<58} {'blur_axis':<47} {'slice':<42} {'entry/T':>8} {'rel-L2':>8} {'cases':>5}")
    for fam in sorted(WORST, key=lambda f: tuple(str(x) for x in f)):
        e, r, c = WORST[fam]
        mark = "" if fam in FAMILIES or not fam[1] else "  (not a FAMILIES key)"
        print(f"{fam[0]:<58} {fam[1]:<47} {str(fam[2]):<42} {e:8.1e} {r:8.1e} {c:5d}{mark}")
    print("overall worst: entry {:.2e}, rel {:.2e} ({} families)".format(max(w[0] for w in WORST.values()),
                                                                         max(w[1] for w in WORST.values()), len(WORST)))


# ---- the cases -------------------------------------------------------------------------------------------------------
# Every family the dispatcher can pick -> the tests that reach it (with the expectation their cases assert)
FAMILIES = {
    (SCAN, SMALL, SLICE_V1): ["test_every_dimension", "test_vd_gates", "test_partial_waves", "test_clouds", "test_entry_points"],
    (SCAN, GENERAL, SLICE_V1): ["test_every_order (vd = 1, order 0 and 4..8, or blur_vpt = 1)"],
    (SCAN, V1, SLICE_V1): ["test_large_m (m > 16384, blur_fuse = 0)", "test_forced_blur_vd1 (blur_small = 0, blur_fuse = 0, vpt 2 / 4)"],
    (SCAN, PAIR_V1_ODD, SLICE_V1): ["test_large_m (d = 8)", "test_forced_blur_vd1 (blur_fuse = 2)"],
    (SCAN, PAIR_V1, SLICE_V1): ["test_forced_blur_vd1 (blur_fuse = 2, d + 1 even)"],
    (SCAN, COMPACT, SLICE_V1): ["test_forced_blur_vd1 (compact_nbr = 2, blur_small = 0)"],
    (SCAN_G1, SMALL, SLICE_V1): ["test_forced_splat (splat_direct = 0)"],
    (SCAN_G, NARROW, VEC): ["test_every_dimension (vd = 3)", "test_vd_gates (vd 2..4)"],
    (SCAN_G, MULTI, VEC): ["test_vd_gates (vd > 512: column tiles)"],
    (SCAN_G, GENERAL, VEC): ["test_forced_splat (splat_group = 0, vd 17..64)", "test_every_order"],
    (SCAN, NARROW, VEC): ["test_row_order (vd = 4, lattice rows, 16-byte aligned)"],
    (GROUP_G, PAIR_NARROW, VEC): ["test_vd_gates (vd 5..16, d + 1 even)"],
    (GROUP_G, PAIR_NARROW_ODD, VEC): ["test_every_dimension (vd = 6, d + 1 odd)", "test_partial_waves"],
    (GROUP_G, NARROW, VEC): ["test_forced_blur_vec (blur_fuse_vec = 0)", "test_entry_points (one-shot filter)"],
    (GROUP_G, GENERAL, VEC): ["test_vd_gates (vd 17..64)", "test_every_order"],
    (SCAN_G, PAIR_NARROW, VEC): ["test_forced_splat (splat_group = 0, vd = 9)"],
    (GROUP, PAIR_NARROW_ODD, VEC): ["test_row_order (vd 8, 12, lattice rows)", "test_apply_affine_dot (lattice rows)"],
    (GROUP, GENERAL, VEC): ["test_apply_affine_dot (vd = 64, lattice rows)"],
    (SCAN, MULTI, VEC): ["test_row_order (vd = 600, lattice rows: column tiles)"],
    (WIDE_G, MULTI, VEC): ["test_vd_gates (vd 65..512)"],
    (WIDE_G, ACTIVE, VEC): ["test_active_rows (blur_active = 2, and a sparse lattice at the default)"],
    (WIDE_G, GENERAL, VEC): ["test_forced_blur_vec (blur_multi = 0 / 2)", "test_every_order (vd = 130)"],
    (WIDE, MULTI, VEC): ["test_row_order (vd = 100, lattice rows)"],
    (SCAN_G, MULTI, VEC_UNPERM): ["test_unpermute_gather (vd = 1000, output > 96 MB)"],
    (GROUP_G, GENERAL, VEC_UNPERM_LDS): ["test_unpermute_gather (vd = 48, output > 96 MB)"],
    (GROUP_G, GENERAL, VEC_UNPERM): ["test_unpermute_gather (vd = 48, perm_rows = 0)"],
    (FIRST_SEQ, SMALL, SLICE_V1): ["test_first_touch_splat (splat_first = 2, isolated points)"],
    (FIRST_SEQ_X, SMALL, SLICE_V1): ["test_first_touch_splat (splat_first = 2, shared vertices)"],
    (FIRST, SMALL, SLICE_V1): ["test_first_touch_splat (splat_first = 3)"],
    (FIRST_X, SMALL, SLICE_V1): ["test_first_touch_splat (splat_first = 3, shared vertices)"],
    (BLOCK, SMALL, SLICE_BLOCK_UNPERM): ["test_block_path (block_path = 2, block_e 16 / 24)"],
    (BLOCK, SMALL, SLICE_BLOCK): ["test_block_path (lattice rows, unpermute_gather = 0)"],
    (SPLAT_ONEHOT, SMALL, SLICE_V1): ["test_onehot (dense stages, vd = 1)"],
    (SPLAT_ONEHOT, PAIR_NARROW_ODD, VEC): ["test_onehot (dense stages, vd 8..16, d + 1 odd)"],
    (SPLAT_ONEHOT, PAIR_NARROW, VEC): ["test_onehot (dense stages, vd 8..16, d + 1 even)"],
    (SPLAT_ONEHOT, NARROW, VEC): ["test_onehot (dense stages, vd = 4, order 2, blur_fuse_vec = 0)"],
    (SPLAT_ONEHOT, V1, SLICE_V1): ["test_onehot (dense stages, vd = 1, m > 16384, order 2)"],
    (SPLAT_ONEHOT, PAIR_V1, SLICE_V1): ["test_onehot (dense stages, vd = 1, m > 16384, d + 1 even)"],
    (SPLAT_ONEHOT, PAIR_V1_ODD, SLICE_V1): ["test_onehot (dense stages, vd = 1, m > 16384, d + 1 odd)"],
    (SEED, OH_PAIR, OH_SLICE): ["test_onehot (frontier, order 1)"],
    (SEED, OH_AXIS, OH_SLICE): ["test_onehot (frontier, order 2, or blur_fuse_vec = 0)"],
    (BACKWARD, MULTI, CONTRACT): ["test_fused_backward_grad_src (grad_src = K g)"],
}
NAMES = {s for fam in FAMILIES for s in fam if s}


def known(fam):
    """Cases without a fixed expectation (the moved hand-run checks) still only run families listed above."""
    assert {s for s in fam if s} <= NAMES, ("a kernel FAMILIES does not name", fam)
    return fam


@pytest.mark.parametrize("d", range(1, 33))
def test_every_dimension(d):
    """d = 1..32: every slice_v1<D1>, every slice_vec<D1> (D1 <= 20) and the run-time slice_vec above, n = 257 (one
    point past a workgroup), at vd = 1 (blur_small), vd = 3 (one partial chunk) and vd = 6 (two chunks, pair blur)."""
    n = 257
    x, l64 = operator("gauss1", n, d, RBF1, seed=d)
    lat = plx.Lattice().build(cuda(x), RBF1)
    try:
        for vd in (1, 3, 6):
            run_apply(lat, l64, rhs(n, vd, d * 10 + vd), expect(vd, d, m=lat.m), ("d", d, vd))
    finally:
        lat.close()


@pytest.mark.parametrize("order", range(9))
def test_every_order(order):
    """Orders 0..8 through the single-column general blur (blur_axis_kernel<float, ORDER>, run-time order above 3; orders
    1..3 with blur_vpt = 1, which leaves the vd = 1 special kernels) and the float4 general blur (vd = 7 and 20: orders 0
    and >= 4 at any width, 1..3 between the narrow and the multi-row kernels; vd = 130 with blur_multi = 0), with
    Gaussian and lopsided (non-symmetric, centre 0.85) taps, at d = 2, 3 and 7."""
    for ti, taps in enumerate((gauss_taps(order), lopsided_taps(order))):
        for d in (2, 3, 7):
            n = 701
            x, l64 = operator("gauss1", n, d, taps, seed=order + d)
            vpt = 1 if 1 <= order <= 3 else 4
            with tuned(blur_vpt=vpt, blur_multi=0):
                lat = plx.Lattice().build(cuda(x), taps)
            try:
                for vd in (1, 7, 20, 130):
                    fam = expect(vd, d, order, m=lat.m, blur_vpt=vpt, blur_multi=0)
                    if vd == 1:
                        assert fam[1] == GENERAL
                    run_apply(lat, l64, rhs(n, vd, order * 100 + vd + ti), fam, ("order", order, ti, d, vd))
            finally:
                lat.close()


VD_GATES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 61, 64, 65, 68, 69, 124, 128, 129, 256, 257, 512, 513, 1000]


def test_vd_gates():
    """vd at every float4 chunk gate (1 | 2-4 | 5-16 | 17-64 | 65-128 | > 128 chunks: scan, lane groups, wide rows of
    one and two chunk slots per lane, column tiles) on one lattice, d = 3, n = 701."""
    n, d = 701, 3
    x, l64 = operator("gauss1", n, d, RBF1, seed=3)
    lat = plx.Lattice().build(cuda(x), RBF1)
    try:
        for vd in VD_GATES:
            run_apply(lat, l64, rhs(n, vd, vd), expect(vd, d, m=lat.m), ("vd", vd))
    finally:
        lat.close()


@pytest.mark.parametrize("n", [1, 2, 63, 65, 701])
def test_partial_waves(n):
    """Few points: partial waves and workgroups in every stage (d = 4: d + 1 odd), at vd 1, 5, 20, 130 and 513."""
    d = 4
    x, l64 = operator("gauss0.3", n, d, RBF1, seed=n)
    lat = plx.Lattice().build(cuda(x), RBF1)
    try:
        for vd in (1, 5, 20, 130, 513):
            run_apply(lat, l64, rhs(n, vd, n + vd), expect(vd, d, m=lat.m), ("n", n, vd))
    finally:
        lat.close()


@pytest.mark.parametrize("kind", ["gauss0.3", "gauss1", "gauss3", "simplex", "isolated", "dup", "grid"])
def test_clouds(kind):
    """Every cloud kind: one simplex (rows of n corners), isolated points (no neighbours), exact duplicates, grid ties
    (points on lattice-aligned spots), at d = 2, 5 and 13."""
    for d in (2, 5, 13):
        n = 1001
        x, l64 = operator(kind, n, d, RBF1, seed=d)
        lat = plx.Lattice().build(cuda(x), RBF1)
        try:
            if kind == "simplex":
                assert lat.m == d + 1
            for vd in (1, 4, 9, 70):
                run_apply(lat, l64, rhs(n, vd, d + vd), expect(vd, d, m=lat.m), ("cloud", kind, d, vd))
        finally:
            lat.close()


def test_large_m():
    """m > 16384 (the single-column blur leaves the one-workgroup kernel): per-axis v1 passes and the two-axes pair blur."""
    n, d = 3000, 8
    x, l64 = operator("gauss3", n, d, RBF1, seed=8)
    for fuse in (0, 1):
        with tuned(blur_fuse=fuse):
            lat = plx.Lattice().build(cuda(x), RBF1)
        try:
            assert lat.m > 16384
            for vd in (1, 9):
                run_apply(lat, l64, rhs(n, vd, vd + fuse), expect(vd, d, m=lat.m, blur_fuse=fuse), ("large m", fuse, vd))
        finally:
            lat.close()


@pytest.mark.parametrize("d", [2, 3, 8])
def test_forced_blur_vd1(d):
    """The single-column blur kernels natural inputs make expensive: per-axis v1 (vpt 2 / 4), the pair blur (d + 1 even
    and odd), the compacted neighbour table (orders 1..3, Gaussian and lopsided taps)."""
    n = 701
    for order in (1, 2, 3):
        for taps in (gauss_taps(order), lopsided_taps(order)):
            x, l64 = operator("gauss1", n, d, taps, seed=d + order)
            v = rhs(n, 1, d * order)
            for sw in ({"blur_small": 0, "blur_fuse": 0, "blur_vpt": 2}, {"blur_small": 0, "blur_fuse": 0, "blur_vpt": 4},
                       {"blur_small": 0, "blur_fuse": 2, "blur_vpt": 2}, {"blur_small": 0, "blur_fuse": 2, "blur_vpt": 4},
                       {"blur_small": 0, "compact_nbr": 2}):
                with tuned(**sw):
                    lat = plx.Lattice().build(cuda(x), taps)
                try:
                    fam = expect(1, d, order, m=lat.m, compact="compact_nbr" in sw, **sw)
                    run_apply(lat, l64, v, fam, ("blur vd1", d, order, sw))
                finally:
                    lat.close()


def test_forced_blur_vec():
    """blur_fuse_vec = 0 (per-axis narrow kernel at 2..4 chunks), blur_multi = 0 / 2 (the general kernel below 32 chunks),
    blur_narrow = 0."""
    n, d = 701, 5
    x, l64 = operator("gauss1", n, d, RBF1, seed=5)
    for sw, vds in (({"blur_fuse_vec": 0}, (5, 16)), ({"blur_multi": 0}, (70, 200)), ({"blur_multi": 2}, (100, 130)),
                    ({"blur_narrow": 0}, (3, 12))):
        with tuned(**sw):
            lat = plx.Lattice().build(cuda(x), RBF1)
        try:
            for vd in vds:
                run_apply(lat, l64, rhs(n, vd, vd), expect(vd, d, m=lat.m, **sw), ("blur vec", sw, vd))
        finally:
            lat.close()


def test_active_rows():
    """The active-row blur (centre tap 1, 17..128 chunks, in place over the vertices that have a neighbour on the axis):
    forced on a Gaussian cloud, and at the default on a lattice with m >= 0.75 n (d + 1) (isolated points: no row
    changes)."""
    n, d = 2001, 6
    for kind, sw in (("gauss1", {"blur_active": 2}), ("gauss3", {"blur_active": 2}), ("isolated", {"blur_active": 1})):
        x, l64 = operator(kind, n, d, RBF1, seed=6)
        with tuned(**sw):
            lat = plx.Lattice().build(cuda(x), RBF1)
        try:
            if sw["blur_active"] == 1:
                assert lat.m >= 0.75 * n * (d + 1)
            for vd in (65, 130, 300, 512):
                run_apply(lat, l64, rhs(n, vd, vd), expect(vd, d, m=lat.m, active=True), ("active", kind, vd))
        finally:
            lat.close()


def test_forced_splat():
    """splat_direct = 0 (vd = 1 gathers into lattice order first), splat_group = 0 (column tiles at 2..16 chunks),
    splat_wide = 0 / 2 (column tiles at 17..128 chunks, and below 32 chunks)."""
    n, d = 701, 3
    x, l64 = operator("gauss1", n, d, RBF1, seed=31)
    for sw, vds in (({"splat_direct": 0}, (1,)), ({"splat_group": 0}, (9, 20, 64)), ({"splat_wide": 0}, (65, 300)),
                    ({"splat_wide": 2}, (100, 130))):
        with tuned(**sw):
            lat = plx.Lattice().build(cuda(x), RBF1)
        try:
            for vd in vds:
                run_apply(lat, l64, rhs(n, vd, vd + 7), expect(vd, d, m=lat.m, **sw), ("splat", sw, vd))
        finally:
            lat.close()


@pytest.mark.parametrize("vertex_order", [0, 2])
def test_row_order(vertex_order):
    """Caller and lattice row order (set_lattice_row_order: no gather in, no scatter out where the rows are whole 16-byte
    vectors), under first-touch and Morton vertex numbering."""
    n, d = 1001, 4
    x, l64 = operator("gauss0.3", n, d, RBF1, seed=44)
    with tuned(vertex_order=vertex_order):
        lat = plx.Lattice().build(cuda(x), RBF1)
    try:
        assert lat.stage_kernels()["vertex_order"] == [["first_touch", None, "morton"][vertex_order]]
        perm = lat.shard_perm()
        for vd in (1, 3, 4, 8, 12, 100, 256, 600):
            v = rhs(n, vd, vd)
            run_apply(lat, l64, v, expect(vd, d, m=lat.m), ("caller rows", vertex_order, vd))
            lat.set_lattice_row_order(True)
            try:
                out = lat.apply(cuda(v)[perm].contiguous())
                fam = ran(lat, expect(vd, d, m=lat.m, lattice_rows=True), ("lattice rows", vertex_order, vd))
            finally:
                lat.set_lattice_row_order(False)
            want, T = reference(l64, v)
            pn = perm.cpu().numpy()
            check(fam, out, want[pn], T[pn], ("lattice rows", vertex_order, vd))
    finally:
        lat.close()


def test_source_layout():
    """A src view 4 bytes past a 16-byte boundary (the lattice-row splat must gather it; the caller-row gather takes its
    per-float form) and a non-contiguous src."""
    n, d = 701, 3
    x, l64 = operator("gauss1", n, d, RBF1, seed=9)
    lat = plx.Lattice().build(cuda(x), RBF1)
    try:
        perm = lat.shard_perm()
        for vd in (4, 8, 100):
            v = rhs(n, vd, vd)
            buf = torch.zeros(n * vd + 4, device="cuda")
            src = buf[1:1 + n * vd].view(n, vd)
            assert src.data_ptr() % 16 == 4
            src.copy_(cuda(v))
            run_apply(lat, l64, v, expect(vd, d, m=lat.m), ("offset src", vd), src=src)
            wide = torch.zeros(n, 2 * vd, device="cuda")
            wide[:, ::2] = cuda(v)
            run_apply(lat, l64, v, expect(vd, d, m=lat.m), ("strided src", vd), src=wide[:, ::2])
            lat.set_lattice_row_order(True)
            try:
                src.copy_(cuda(v)[perm])
                out = lat.apply(src)
                fam = ran(lat, expect(vd, d, m=lat.m, lattice_rows=True, aligned=False), ("offset src, lattice rows", vd))
            finally:
                lat.set_lattice_row_order(False)
            want, T = reference(l64, v)
            pn = perm.cpu().numpy()
            check(fam, out, want[pn], T[pn], ("offset src, lattice rows", vd))
    finally:
        lat.close()


def test_unpermute_gather():
    """Caller row order on outputs over 96 MB: slice into lattice order, then gather the rows out (the LDS-transposed form
    for <= 48 columns; the per-chunk form above, or with perm_rows = 0)."""
    for n, vd, sw in ((530_001, 48, {}), (530_001, 48, {"perm_rows": 0}), (25_301, 1000, {})):
        x, l64 = operator("gauss1", n, 2, RBF1, seed=vd)
        with tuned(**sw):
            lat = plx.Lattice().build(cuda(x), RBF1)
        try:
            run_apply(lat, l64, rhs(n, vd, 5), expect(vd, 2, m=lat.m, n=n, **sw), ("unpermute", n, vd, sw))
        finally:
            lat.close()


def test_first_touch_splat():
    """The first-touch splat (plx_first.hip) forced on: contiguous runs under first-touch numbering (splat_first = 2) and
    scattered stores (3), with and without extra corners (vertices shared between points)."""
    d = 5
    for kind, n in (("isolated", 301), ("gauss1", 701), ("dup", 701)):
        x, l64 = operator(kind, n, d, RBF1, seed=55)
        for mode in (2, 3):
            with tuned(splat_first=mode, vertex_order=0):
                lat = plx.Lattice().build(cuda(x), RBF1)
            try:
                extras = lat.m < n * (d + 1)
                fam = ({2: FIRST_SEQ, 3: FIRST}[mode] + ("+splat_extras_kernel" if extras else ""), SMALL, SLICE_V1)
                v = rhs(n, 1, mode)
                run_apply(lat, l64, v, fam, ("first", kind, mode))
                lat.set_lattice_row_order(True)
                try:
                    perm = lat.shard_perm()
                    out = lat.apply(cuda(v)[perm].contiguous())
                    ran(lat, fam, ("first, lattice rows", kind, mode))
                finally:
                    lat.set_lattice_row_order(False)
                want, T = reference(l64, v)
                pn = perm.cpu().numpy()
                check(fam, out, want[pn], T[pn], ("first, lattice rows", kind, mode))
            finally:
                lat.close()


@pytest.mark.parametrize("block_e", [16, 24])
def test_block_path(block_e):
    """vd = 1 through the block tables (block_path = 2): caller rows (slice into lattice order + unpermute), lattice rows
    and unpermute_gather = 0 (the slice scatters itself); n not a multiple of the block."""
    for n, d, kind in ((4099, 2, "gauss1"), (2001, 7, "gauss0.3"), (2001, 3, "simplex")):
        x, l64 = operator(kind, n, d, RBF1, seed=block_e)
        v = rhs(n, 1, n)
        for ug in (1, 0):
            with tuned(block_path=2, block_e=block_e, unpermute_gather=ug):
                lat = plx.Lattice().build(cuda(x), RBF1)
            try:
                run_apply(lat, l64, v, (BLOCK, SMALL, SLICE_BLOCK_UNPERM if ug else SLICE_BLOCK), ("block", n, d, ug))
                assert lat.block_rows > 0
                if ug:
                    lat.set_lattice_row_order(True)
                    try:
                        perm = lat.shard_perm()
                        out = lat.apply(cuda(v)[perm].contiguous())
                        ran(lat, (BLOCK, SMALL, SLICE_BLOCK), ("block, lattice rows", n, d))
                    finally:
                        lat.set_lattice_row_order(False)
                    want, T = reference(l64, v)
                    pn = perm.cpu().numpy()
                    check((BLOCK, SMALL, SLICE_BLOCK), out, want[pn], T[pn], ("block, lattice rows", n, d))
            finally:
                lat.close()


def test_entry_points():
    """splat -> blur -> slice called one by one, the one-shot plx.filter (single-use dispatch: no pair tables) and
    apply_affine = a K v + b v for two (a, b)."""
    for d, kind in ((3, "gauss1"), (6, "gauss0.3"), (21, "gauss1")):
        n = 901
        x, l64 = operator(kind, n, d, RBF1, seed=d)
        lat = plx.Lattice().build(cuda(x), RBF1)
        try:
            for vd in (1, 6, 130):
                v = rhs(n, vd, vd + d)
                want, T = reference(l64, v)
                vals = lat.splat(cuda(v))
                blurred = lat.blur(vals, vd=vd)
                out = lat.slice(blurred, vd=vd)
                check(ran(lat, expect(vd, d, m=lat.m), ("stages", d, vd)), out, want, T, ("stages", d, vd))
                for a, b in ((0.7, 0.3), (-1.3, 2.5)):
                    out = lat.apply_affine(cuda(v), torch.tensor([a, b], device="cuda"))
                    fam = ran(lat, expect(vd, d, m=lat.m), ("affine", d, vd, a))
                    check(fam, out, a * want + b * v, abs(a) * T + abs(b) * np.abs(v), ("affine", d, vd, a))
                once = plx.filter(cuda(v), cuda(x), RBF1)
                fam = ran(plx.lattice._scratch_lattice(once.device), expect(vd, d, m=l64.m, single_use=True),
                          ("one-shot", d, vd))
                check(fam, once, want, T, ("one-shot", d, vd))
        finally:
            lat.close()


DOT_VD = [2, 3, 5, 16, 17, 64, 65, 255, 256]


@pytest.mark.parametrize("lattice_rows", [False, True])
def test_apply_affine_dot(lattice_rows):
    """The CG step's a K v + b v with the column dots <v, out> formed inside the slice kernel (and left as per-tile
    partials for want_dot = "partial"): the output per entry, the dots against the float64 <v, K64-affine v> in units
    of sum |v| |out| (DOT)."""
    n, d = 2001, 4
    x, l64 = operator("gauss0.3", n, d, RBF1, seed=77)
    lat = plx.Lattice().build(cuda(x), RBF1)
    lat.set_lattice_row_order(lattice_rows)
    pn = lat.shard_perm().cpu().numpy() if lattice_rows else np.arange(n)
    try:
        for vd in DOT_VD:
            v = rhs(n, vd, vd)
            want, T = reference(l64, v)
            a, b = 0.9, 0.35
            want, T, v = (a * want + b * v)[pn], (abs(a) * T + b * np.abs(v))[pn], v[pn]
            ss = torch.tensor([a, b], device="cuda")
            out, dot = lat.apply_affine(cuda(v), ss, want_dot=True)
            fam = ran(lat, expect(vd, d, m=lat.m, lattice_rows=lattice_rows, dot=True), ("dot", vd))
            check(fam, out, want, T, ("dot out", vd))
            dwant = (v.astype(np.float64) * want).sum(0)
            dterms = (np.abs(v) * np.abs(want)).sum(0)
            dratio = float(np.max(np.abs(dot.cpu().numpy() - dwant) / dterms))
            row = WORST.setdefault(("apply_affine_dot: <v, out>", "", ""), [0.0, 0.0, 0])
            row[0], row[2] = max(row[0], dratio), row[2] + 1
            assert dratio <= DOT, ("dot", vd, dratio)
            out2, work, tiles = lat.apply_affine(cuda(v), ss, want_dot="partial")
            assert torch.equal(out2, out)
            vdp = lat.values_stride(vd)
            part = work[:tiles * vdp].view(tiles, vdp).cpu().numpy().astype(np.float64).sum(0)[:vd]
            pratio = float(np.max(np.abs(part - dwant) / dterms))
            row[0] = max(row[0], pratio)
            assert pratio <= DOT, ("partial dots", vd, pratio)
    finally:
        lat.close()


@pytest.mark.parametrize("d", [2, 3, 8, 16, 17, 20])
def test_onehot(d):
    """filter_onehot (kernel rows K e_p on the frontier of their non-zero vertex rows; onehot_slice<D1> up to D1 = 17,
    run-time above) and splat_onehot + blur + slice, for 1..16 candidates, against the matching columns of K64: every
    entry outside the columns' reach must be exactly 0.  Order 1 (pair passes) and 2 (single axes), blur_fuse_vec = 0,
    a sparse and a dense frontier (fine and coarse cloud)."""
    for kind, order, sw in (("gauss1", 1, {}), ("gauss0.3", 2, {}), ("gauss0.3", 1, {"blur_fuse_vec": 0}),
                            ("gauss3", 1, {})):
        n = 1001
        taps = gauss_taps(order)
        x, l64 = operator(kind, n, d, taps, seed=d + order)
        K = l64.matrix()
        with tuned(**sw):
            lat = plx.Lattice().build(cuda(x), taps)
        try:
            perm = lat.shard_perm().cpu().numpy()
            frontier = torch.zeros(1, dtype=torch.int32, device="cuda")
            rng = np.random.default_rng(d * 3 + order)
            for vd, nb in ((1, 1), (4, 3), (8, 8), (12, 12), (16, 13), (16, 16)):
                pts = rng.choice(n, nb, replace=False).astype(np.int32)
                if nb >= 3:
                    pts[1] = (pts[0] + 1) % n              # neighbours in lattice order share vertices
                    pts[2] = pts[0]                        # and the same point twice
                cols = perm[pts]
                e = np.zeros((n, vd), np.float32)
                e[cols, np.arange(nb)] = 1.0
                want = np.zeros((n, vd))
                want[:, :nb] = K[:, cols]
                T = l64.terms64(e)
                ptc = torch.from_numpy(pts).cuda()
                vals, scratch = lat.new_values(vd), lat.new_values(vd)
                for sparse in (True, False):
                    out = torch.full((n, vd), 7.0, device="cuda")
                    lat.filter_onehot(ptc, nb, vals, scratch, out, vd=vd, sparse=sparse, frontier=frontier)
                    if sparse:
                        fam = (SEED, OH_PAIR if order == 1 and not sw else OH_AXIS, OH_SLICE)
                    else:
                        fam = (SPLAT_ONEHOT,) + expect(vd, d, order, m=lat.m, **sw)[1:]
                    check(ran(lat, fam, ("onehot", kind, d, order, vd, nb, sparse)), out, want, T,
                          ("onehot", kind, d, order, vd, nb, sparse))
                # splat_onehot then blur and slice through the stage calls
                v0 = lat.splat_onehot(ptc, nb, lat.new_values(vd), vd=vd)
                out = lat.slice(lat.blur(v0, vd=vd), vd=vd)
                fam = (SPLAT_ONEHOT,) + expect(vd, d, order, m=lat.m, **sw)[1:]
                check(ran(lat, fam, ("splat_onehot", kind, d, vd, nb)), out, want, T, ("splat_onehot", kind, d, vd, nb))
        finally:
            lat.close()


def test_sharded_rows():
    """build(shard = (r, 3)): each shard splats its own rows, the splats add up, each shard slices its own rows: the
    matching rows of K64 v."""
    from simplex_gp_amd.distributed import shard_bounds
    for n, d, vd in ((2003, 3, 1), (2003, 5, 6), (701, 2, 130)):
        x, l64 = operator("gauss0.3", n, d, RBF1, seed=n + d)
        v = rhs(n, vd, d)
        want, T = reference(l64, v)
        lats = [plx.Lattice().build(cuda(x), RBF1, shard=(r, 3)) for r in range(3)]
        try:
            total = None
            for r, lat in enumerate(lats):
                lo, hi = shard_bounds(n, 3, r)
                part = lat.splat(cuda(v[lo:hi]))
                total = part.clone() if total is None else total + part
            for r, lat in enumerate(lats):
                lo, hi = shard_bounds(n, 3, r)
                out = lat.slice(lat.blur(total.clone(), vd=vd), vd=vd)
                fam = ran(lat, expect(vd, d, m=lat.m), ("shard", n, d, vd, r))
                check(fam, out, want[lo:hi], T[lo:hi], ("shard", n, d, vd, r))
        finally:
            for lat in lats:
                lat.close()


def test_fused_backward_grad_src():
    """The fused position gradient's splat of the stacked matrix: its grad_src = K g (the first L filtered columns)."""
    from tests.lattice64 import contract64, stack64
    dk = plx.DiscretizedKernelFN(plx.rbf, 1)
    taps = dk.get_deriv_coeffs().numpy()
    for d, L in ((3, 16), (5, 12)):
        assert plx.Lattice.backward_fusable(L, d)
        n = 1001
        x, l64 = operator("gauss0.3", n, d, taps, seed=d)
        rng = np.random.default_rng(L)
        g, s = rng.standard_normal((n, L)).astype(np.float32), rng.standard_normal((n, L)).astype(np.float32)
        lat = plx.Lattice().build(cuda(x), taps)
        try:
            _, gs = lat.apply_backward(cuda(g), cuda(s), cuda(x))
            fam = ran(lat, (BACKWARD, expect(2 * L * (1 + d), d, m=lat.m)[1], CONTRACT), ("backward", d, L))
            want, T = reference(l64, g)
            check(fam, gs, want, T, ("backward grad_src", d, L))
            assert rel_l2(contract64(g, s, x, l64.apply(stack64(g, s, x)))[1], want) <= 1e-12
        finally:
            lat.close()


# ---- the hand-run checks, moved in (tests/checks/extreme_shapes.py, tests/checks/fuzz_filter.py) ----------------------
EXTREME = [(500, 32, 1, 1), (500, 32, 5, 2), (2000, 25, 3, 3), (300, 31, 130, 1), (1000, 3, 1, 4), (1000, 3, 7, 5),
           (1000, 2, 40, 6), (1000, 4, 1, 8), (700, 5, 130, 7), (64, 1, 1, 8)]


@pytest.mark.parametrize("n,d,vd,order", EXTREME)
def test_extreme_shapes(n, d, vd, order):
    """d up to 32 and orders up to 8 (PLX_MAX_ORDER) through the one-shot filter and a many-MVM build with Morton vertex
    numbering forced."""
    rng = np.random.default_rng(n + d + vd + order)
    x = (rng.standard_normal((n, d)) * 0.8).astype(np.float32)
    v = rng.standard_normal((n, vd)).astype(np.float32)
    taps = gauss_taps(order)
    l64 = Lattice64(x, taps)
    want, T = reference(l64, v)
    got = plx.filter(cuda(v), cuda(x), taps)
    check(known(family_of(plx.lattice._scratch_lattice(got.device))), got, want, T, ("extreme one-shot", n, d, vd, order))
    with tuned(vertex_order=2):
        lat = plx.Lattice().build(cuda(x), taps)
    try:
        out = lat.apply(cuda(v))
        assert lat.stage_kernels()["vertex_order"] == ["morton"] or lat.m < 2
        check(known(family_of(lat)), out, want, T, ("extreme morton", n, d, vd, order))
    finally:
        lat.close()


def fuzz_case(c, rng):
    """One case of tests/checks/fuzz_filter.py's generator (shapes, column counts, orders, scales, cloud kinds)."""
    n = int(rng.choice([1, 2, 3, 17, 64, 65, 255, 257, 1000, 2049]))
    d = int(rng.integers(1, 13))
    vd = int(rng.choice([1, 1, 2, 3, 4, 5, 6, 7, 9, 12, 13, 16, 17, 31, 33, 60, 64, 65, 100, 124, 126, 130, 198, 260]))
    order = int(rng.integers(0, 4))
    scale = float(rng.choice([0.02, 0.3, 1.0, 4.0, 30.0]))
    kind = str(rng.choice(["normal", "grid", "dup", "line", "same"]))
    if kind == "normal":
        ref = rng.standard_normal((n, d))
    elif kind == "grid":
        ref = rng.integers(-3, 4, (n, d)).astype(np.float64) * 0.5
    elif kind == "dup":
        k = max(1, n // 20)
        ref = rng.standard_normal((k, d))[rng.integers(0, k, n)]
    elif kind == "line":
        ref = np.outer(rng.standard_normal(n), rng.standard_normal(d))
    else:
        ref = np.tile(rng.standard_normal((1, d)), (n, 1))
    ref = (ref * scale).astype(np.float32)
    src = rng.standard_normal((n, vd)).astype(np.float32)
    taps = np.array([0.1, 0.3, 0.6, 1.0, 0.6, 0.3, 0.1][3 - order: 4 + order], np.float32)
    return ref, src, taps


def test_fuzz_fixed_seed():
    """30 fixed-seed cases of the fuzz generator: odd ones through build + apply with Morton numbering and both
    two-axes blurs forced, even ones through the one-shot filter; the compacted neighbour table on every third, the
    shipped switches otherwise."""
    rng = np.random.default_rng(7)
    for c in range(30):
        ref, src, taps = fuzz_case(c, rng)
        l64 = Lattice64(ref, taps)
        want, T = reference(l64, src)
        sw = dict(DEFAULTS, compact_nbr=2 if c % 3 == 0 else 1)
        if c % 2:
            with tuned(**dict(sw, vertex_order=2, blur_fuse=2)):
                lat = plx.Lattice().build(cuda(ref), taps)
            try:
                out = lat.apply(cuda(src))
                fam = known(family_of(lat))
            finally:
                lat.close()
        else:
            with tuned(**sw):
                out = plx.filter(cuda(src), cuda(ref), taps)
                fam = known(family_of(plx.lattice._scratch_lattice(out.device)))
        check(fam, out, want, T, ("fuzz", c, ref.shape, src.shape[1], taps.size))


def test_every_family_was_reached():
    """Acceptance: every family in FAMILIES ran in this module (run it whole: pytest -m gpu tests/test_forward_fp64.py)."""
    missing = [f for f in FAMILIES if f not in REACHED]
    if len(REACHED) == 0:
        pytest.fail("no case of this module ran before the acceptance test")
    assert not missing, missing
