"""The block splat and slice (plx_block.hip) at every edge of their staging loops, against float64.

slice_block_kernel stages the values of a block's rows in batches of 8 passes of kBlkT = 256 rows, with the threads past
the last row repeating it; splat_block_kernel stages its source window in up to kBlkMaxP / kBlkT = 4 passes of 256
points; splat_combine_kernel gathers four block rows per lane as one batch.  The clouds below put a block on every edge
of those loops: rows per block from below one pass to past two batches, a last block with fewer points than threads,
with exactly one pass, with one pass and a few points, and windows of 2, 3 and the full 4 passes.
test_the_clouds_reach_every_loop_edge recomputes the block geometry on the host with the numpy model of the point order
(tests/test_point_order_cell.py) and fails if a later change of the geometry moves the clouds off those edges.

The reference is the float64 operator of tests/lattice64.py and the bars are those of tests/test_forward_fp64.py (its
`reference` and `check`, imported; its `operator` draws its clouds from tests/lattice64.cloud, these come from a torch
generator like those of tests/test_point_order_cell.py, so the Lattice64 is built here).
"""
import contextlib

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import test_forward_fp64 as fp
from tests.lattice64 import Lattice64
from tests.test_point_order_cell import BLK_T, block_points, fixed_cells, order_keys

RBF1 = fp.RBF1
ROW_BATCH = 8 * BLK_T                       # plx_block.hip: kSliceBatch passes of kBlkT rows

CLOUDS = {                                  # name: (n, d, lengthscale)
    "d8": (50_000, 8, 1.0),
    "d8_small": (1_000, 8, 2.0),
    "d4": (9_001, 4, 1.0),
    "d2": (3_000, 2, 1.0),
    "d6": (40_000, 6, 0.6),
}
# What the model gives (block_e 16, 24): points per block, blocks, points of the last block, fewest and most rows of a block
GEOMETRY = {
    ("d8", 16): dict(P=448, blocks=112, last=272, rows=(685, 2923)),
    ("d8", 24): dict(P=672, blocks=75, rows=(1220, 4262)),
    ("d8_small", 16): dict(blocks=3, last=104),
    ("d8_small", 24): dict(blocks=2, last=328),
    ("d4", 16): dict(P=816, last=25, rows=(31, 556)),
    ("d4", 24): dict(P=1008, last=937),
    ("d2", 16): dict(P=1024, rows=(23, 48)),
    ("d2", 24): dict(P=1008),
    ("d6", 16): dict(P=576, last=256),
    ("d6", 24): dict(P=864, last=256),
}
_HOST = {}
_REF = {}
_PLAIN = {}


def positions(name):
    n, d, ell = CLOUDS[name]
    g = torch.Generator().manual_seed(1234)
    return (torch.randn(n, d, generator=g) / ell).contiguous()


def host(name):
    """The cloud, its oracle embedding and the model's point order, once per module."""
    if name not in _HOST:
        x = positions(name)
        oracle.set_exact_mode(False)
        try:
            o = oracle.Lattice(x.numpy(), RBF1)
            greedy, ev, m = o.greedy.copy(), o.entry_vertex.astype(np.int64), int(o.m)
            o.close()
        finally:
            oracle.set_exact_mode(True)
        perm = np.argsort(order_keys(fixed_cells(greedy)), kind="stable")
        _HOST[name] = dict(x=x, ev=ev, m=m, perm=perm)
    return _HOST[name]


def geometry(name, e):
    """dict(P, blocks, last, rows = per-block row counts, m, nnz) of the model for block_e = e."""
    h = host(name)
    n, d, _ = CLOUDS[name]
    P = block_points(e, d + 1)
    ev = h["ev"][h["perm"]]
    rows = np.array([len(np.unique(ev[p0:p0 + P])) for p0 in range(0, n, P)])
    return dict(P=P, blocks=len(rows), last=n - (len(rows) - 1) * P, rows=rows, m=h["m"], nnz=n * (d + 1))


def reference64(name, v):
    if name not in _REF:
        l64 = Lattice64(host(name)["x"].numpy(), RBF1)
        _REF[name] = (l64,) + fp.reference(l64, v)
    return _REF[name]


@contextlib.contextmanager
def switches(**sw):
    """Process-wide plx_tune switches around a build; back to the shipped defaults afterwards."""
    fp.set_switches(sw)
    try:
        yield
    finally:
        fp.set_switches({k: fp.DEFAULTS[k] for k in sw})


@contextlib.contextmanager
def own_books():
    """fp.check keeps the forward module's per-family worst figures and its reached set: leave both as they were, so
    that its acceptance test counts only its own cases."""
    worst, reached = {k: list(v) for k, v in fp.WORST.items()}, set(fp.REACHED)
    try:
        yield
    finally:
        fp.WORST.clear(); fp.WORST.update(worst)
        fp.REACHED.clear(); fp.REACHED.update(reached)


def plain(name):
    """The same cloud built with block_path = 0 (slice_v1_kernel), once per module."""
    if name not in _PLAIN:
        with switches(block_path=0):
            _PLAIN[name] = fp.plx.Lattice().build(host(name)["x"].cuda(), RBF1)
    return _PLAIN[name]


# ---- host only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLOUDS))
def test_the_clouds_reach_every_loop_edge(name):
    """The model's block geometry of every cloud is the one the cases below were chosen for."""
    for e in (16, 24):
        g = geometry(name, e)
        want = GEOMETRY[(name, e)]
        print(f"{name}, block_e {e}: P {g['P']}, {g['blocks']} blocks, last {g['last']} points, "
              f"rows per block {g['rows'].min()}..{g['rows'].max()}, m {g['m']}")
        # the block path is chosen without being forced
        assert 2 * g["m"] <= g["nnz"] and 10 * int(g["rows"].sum()) <= 7 * g["nnz"]
        for key in ("P", "blocks", "last"):
            if key in want:
                assert g[key] == want[key], (name, e, key, g[key])
        if "rows" in want:
            assert (g["rows"].min(), g["rows"].max()) == want["rows"], (name, e, g["rows"].min(), g["rows"].max())
    g16, g24 = geometry(name, 16), geometry(name, 24)
    if name == "d8":        # 3 to 17 passes of 256 rows, across one and two row batches; a last block of one pass + 16
        assert g16["rows"].max() > ROW_BATCH and g24["rows"].max() > 2 * ROW_BATCH and g24["rows"].min() < ROW_BATCH
        assert g16["last"] == BLK_T + 16
        assert -(-g16["P"] // BLK_T) == 2 and -(-g24["P"] // BLK_T) == 3
    elif name == "d8_small":  # a last block with fewer points than threads
        assert g16["last"] < BLK_T < g24["last"] < 2 * BLK_T
    elif name == "d4":        # four window elements per thread, blocks with fewer rows than threads
        assert -(-g16["P"] // BLK_T) == 4 and -(-g24["P"] // BLK_T) == 4
        assert g16["rows"].min() < BLK_T < g16["rows"].max() and g16["last"] < 64
    elif name == "d2":        # the full 4 x 256 window
        assert g16["P"] == 4 * BLK_T and g16["rows"].max() < 64
    elif name == "d6":        # a pass with zero remainder
        assert g16["last"] == BLK_T and g24["last"] == BLK_T


# ---- on the GPU -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("block_e", [16, 24])
@pytest.mark.parametrize("name", list(CLOUDS))
def test_block_chains(name, block_e):
    """Lattice.apply through the block kernels in caller and in lattice row order against float64, bit-equal when
    repeated, and the block slice bit-equal to slice_v1_kernel on the same vertex values."""
    n, d, _ = CLOUDS[name]
    x = host(name)["x"]
    v = fp.rhs(n, 1, n + d)
    l64, want, T = reference64(name, v)
    with switches(block_e=block_e):
        lat = fp.plx.Lattice().build(x.cuda(), RBF1)
        lat.prepare(1)
    try:
        assert lat.m == l64.m
        g = geometry(name, block_e)
        assert lat.block_rows == int(g["rows"].sum())          # the block path was chosen, with the model's geometry
        src = fp.cuda(v)
        pt = lat.shard_perm()
        pn = pt.cpu().numpy()
        with own_books():
            out = lat.apply(src)
            k = lat.stage_kernels(1)
            assert "splat_block_kernel" in k["splat"] and "slice_block_kernel" in k["slice"], k
            fp.check(fp.family_of(lat), out, want, T, ("caller rows", name, block_e))
            assert torch.equal(lat.apply(src), out)
            lat.set_lattice_row_order(True)
            try:
                src_l = src[pt].contiguous()
                out_l = lat.apply(src_l)
                k = lat.stage_kernels(1)
                assert "splat_block_kernel" in k["splat"] and k["slice"] == ["slice_block_kernel"], k
                fp.check(fp.family_of(lat), out_l, want[pn], T[pn], ("lattice rows", name, block_e))
                assert torch.equal(lat.apply(src_l), out_l)
            finally:
                lat.set_lattice_row_order(False)
        # the slice alone, on the blurred vertex values of this input, against the per-point kernel
        ref_lat = plain(name)
        assert ref_lat.m == lat.m and ref_lat.stage_kernels()["vertex_order"] == lat.stage_kernels()["vertex_order"]
        values = lat.blur(lat.splat(src), vd=1)
        for rows_on in (False, True):
            lat.set_lattice_row_order(rows_on)
            ref_lat.set_lattice_row_order(rows_on)
            try:
                got = lat.slice(values, vd=1)
                assert "slice_block_kernel" in lat.stage_kernels(1)["slice"]
                ref = ref_lat.slice(values, vd=1)
                assert ref_lat.stage_kernels(1)["slice"] == ["slice_v1_kernel"]
                assert torch.equal(got, ref), ("slice", name, block_e, rows_on)
            finally:
                lat.set_lattice_row_order(False)
                ref_lat.set_lattice_row_order(False)
    finally:
        lat.close()
