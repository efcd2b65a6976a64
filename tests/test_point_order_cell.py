"""The point order: a stable sort by (shard, Z-interleaved coordinates of the cell a point is embedded in).

The build orders the points by the cell of their fixed-up nearest zero-colour vertex (plx_build.hip: nearest_vertex,
order_coords, coord_range_kernel, sortkey_kernel), the same vertex embed_kernel stores in the point record.  The numpy
model below forms that key from the CPU oracle's embedding: the cell from oracle.Lattice(...).greedy, the coordinate
ranges (every 8th point from 2^16 points on), the clamp to the range, the dropped low bits past 62 key bits, the shard
head bits and the Z-interleave.  The tests check that Lattice.shard_perm() is a stable sort of the model's key, and that
the number of block rows equals the model's count of distinct (block, vertex) pairs under that order and lies below the
count the same cloud gives when ordered by the plainly rounded coordinates (the key of earlier versions).
"""
import numpy as np
import pytest
import torch

from oracle import oracle

RBF1 = np.array([0.34608543, 1.0, 0.34608543], np.float32)

# plx_build.hip: kMaxOrderCoords, kOrderSample, kOrderSampleMinPoints, kBlock;  plx_block.hip: kBlkT, kBlkMaxP
MAX_ORDER_COORDS, ORDER_SAMPLE, ORDER_SAMPLE_MIN_POINTS, BLOCK_THREADS = 16, 8, 1 << 16, 256
BLK_T, BLK_MAX_P = 256, 1024


# ---- the model ------------------------------------------------------------------------------------------------------
def elevate(x, sf):
    """Elevated coordinates [n, d+1] in float32, in the association order of the library (and of the reference)."""
    x = np.asarray(x, np.float32)
    n, d = x.shape
    f = np.float32
    el = np.empty((n, d + 1), np.float32)
    el[:, d] = f(-d) * x[:, d - 1] * sf[d - 1]
    for i in range(d - 1, 0, -1):
        el[:, i] = (el[:, i + 1] - f(i) * x[:, i - 1] * sf[i - 1]) + f(i + 2) * x[:, i] * sf[i]
    el[:, 0] = el[:, 1] + f(2) * x[:, 0] * sf[0]
    return el


def rounded_cells(x, taps):
    """[n, d+1] plainly rounded elevated coordinates in units of d+1: no fix-up (they need not sum to zero)."""
    d = x.shape[1]
    el = elevate(x, oracle.scale_factors(d, taps))
    return np.rint(el * (np.float32(1.0) / np.float32(d + 1))).astype(np.int64)


def fixed_cells(greedy):
    """[n, d+1] cell of the fixed-up nearest zero-colour vertex in units of d+1 (exact: greedy holds multiples of d+1)."""
    g = np.asarray(greedy, np.int64)
    d1 = g.shape[1]
    assert not (g % d1).any() and not g.sum(1).any()
    return g // d1


def key_layout(q, n_shards):
    """(lo, bits, drop, shard_bits) as the build lays the key out from the (sampled) coordinate ranges."""
    n = q.shape[0]
    nc = min(q.shape[1], MAX_ORDER_COORDS)
    stride = ORDER_SAMPLE if n >= ORDER_SAMPLE_MIN_POINTS else 1
    rows = np.arange(0, n, stride)
    if len(rows) % BLOCK_THREADS:            # the padding threads of the last workgroup repeat the last point
        rows = np.append(rows, n - 1)
    lo = q[rows, :nc].min(0)
    span = q[rows, :nc].max(0) - lo
    bits = np.array([int(s).bit_length() for s in span])
    drop = np.zeros(nc, np.int64)
    shard_bits = (n_shards - 1).bit_length()
    while bits.sum() + shard_bits > 62:       # the widest coordinate (the first of them) gives up its lowest bit
        w = int(np.argmax(bits))
        if bits[w] == 0:
            break
        bits[w] -= 1
        drop[w] += 1
    return lo, bits, drop, shard_bits


def order_keys(q, n_shards=1):
    """uint64 sort key of every point from its cell coordinates q [n, d+1]."""
    n = q.shape[0]
    lo, bits, drop, _ = key_layout(q, n_shards)
    nc = len(bits)
    v = np.clip((q[:, :nc] - lo) >> drop, 0, (1 << bits) - 1).astype(np.uint64)
    base, extra = divmod(n, n_shards)
    p = np.arange(n, dtype=np.int64)
    split = (base + 1) * extra
    shard = np.where(p < split, p // (base + 1), extra + (p - split) // max(base, 1)) if n_shards > 1 else np.zeros(n, np.int64)
    key = shard.astype(np.uint64)
    for b in range(int(bits.max(initial=0)) - 1, -1, -1):
        for c in range(nc):
            if bits[c] > b:
                key = (key << np.uint64(1)) | ((v[:, c] >> np.uint64(b)) & np.uint64(1))
    return key


def block_points(e, d1):
    mult = 48 if e == 24 else 16
    return min((BLK_T * e // d1) // mult * mult, BLK_MAX_P // mult * mult)


def count_block_rows(perm, entry_vertex, P):
    """Distinct (block, vertex) pairs over blocks of P consecutive points in the order `perm`."""
    ev = np.asarray(entry_vertex, np.int64)[perm]
    blk = (np.arange(len(perm), dtype=np.int64) // P)[:, None]
    return len(np.unique((blk * (ev.max() + 1) + ev).ravel()))


# ---- host only ------------------------------------------------------------------------------------------------------
def test_key_model_on_a_hand_made_cloud():
    """d = 2 (cells in units of 3).  With unit scale factors the elevated point of x is (x0 + x1, x1 - x0, -2 x1).
    Point B = (-0.05, 1.65) elevates to (1.6, 1.7, -3.3): rounded to multiples of 3 that is (3, 3, -3), which sums to 3,
    not 0, so one coordinate has to come down.  The residuals are (-1.4, -1.3, -0.3); the smallest (coordinate 0) has
    the highest rank and wraps: the fixed-up vertex is (0, 3, -3), cell (0, 1, -1), where plain rounding says (1, 1, -1).
    Point A = (0.05, 0.25) elevates to (0.3, 0.2, -0.5) and rounds to (0, 0, 0) either way."""
    sf = np.ones(2, np.float32)
    x = np.array([[0.05, 0.25], [-0.05, 1.65]], np.float32)
    el = elevate(x, sf)
    np.testing.assert_allclose(el, [[0.3, 0.2, -0.5], [1.6, 1.7, -3.3]], atol=1e-6)
    rounded = np.rint(el * (np.float32(1.0) / np.float32(3))).astype(np.int64)
    assert rounded.tolist() == [[0, 0, 0], [1, 1, -1]] and rounded[1].sum() != 0
    # the fix-up by hand, as the embedding does it
    greedy = rounded * 3
    s = greedy.sum(1) // 3
    assert s.tolist() == [0, 1]
    df = el[1] - greedy[1]
    rank = np.array([(df[i] < df).sum() for i in range(3)])        # rank = how many residuals are larger
    assert rank.tolist() == [2, 1, 0]
    greedy[1] -= np.where(rank >= 3 - s[1], 3, 0)
    assert greedy.tolist() == [[0, 0, 0], [0, 3, -3]]
    q = fixed_cells(greedy)
    assert q.tolist() == [[0, 0, 0], [0, 1, -1]]
    # the layout: coordinate 0 is constant (0 bits), 1 spans 0..1 (1 bit), 2 spans -1..0 (1 bit, lo = -1)
    lo, bits, drop, shard_bits = key_layout(q, 1)
    assert (lo.tolist(), bits.tolist(), drop.tolist(), shard_bits) == ([0, 0, -1], [0, 1, 1], [0, 0, 0], 0)
    # key = (bit of coordinate 1, bit of coordinate 2): A = (0, 1) = 1, B = (1, 0) = 2
    assert order_keys(q).tolist() == [1, 2]
    # the rounded key has a bit for coordinate 0 too: A = (0, 0, 1) = 1, B = (1, 1, 0) = 6
    assert order_keys(rounded).tolist() == [1, 6]
    # two shards of one point each: the shard id leads
    assert order_keys(q, n_shards=2).tolist() == [1, (1 << 2) | 2]


def test_key_model_clamps_and_drops_bits():
    """A point outside the sampled range takes the outermost cell; past 62 key bits the widest coordinate loses low bits."""
    n = ORDER_SAMPLE_MIN_POINTS + ORDER_SAMPLE * BLOCK_THREADS          # sampled, and no padding thread: n - 1 is not sampled
    q = np.zeros((n, 2), np.int64)
    q[::ORDER_SAMPLE, 0] = np.arange(n // ORDER_SAMPLE) % 4             # sampled range 0..3
    q[1, 0], q[3, 0] = 9, -5                                            # unsampled outliers
    k = order_keys(q)
    assert k[1] == 3 and k[3] == 0 and k.max() == 3
    wide = np.zeros((4, 3), np.int64)
    wide[1] = [(1 << 30) - 1, (1 << 20) - 1, (1 << 20) - 1]
    lo, bits, drop, _ = key_layout(wide, 1)
    assert bits.tolist() == [22, 20, 20] and drop.tolist() == [8, 0, 0]


# ---- on the GPU -----------------------------------------------------------------------------------------------------
SHAPES = {                                   # name: (n, d, lengthscale, shard)
    "d4": (50_000, 4, 1.0, None),            # below kOrderSampleMinPoints: exact ranges
    "d6": (60_000, 6, 1.0, None),
    "d8_sampled": (70_000, 8, 2.0, None),    # ranges from every 8th point: clamping
    "d4_shard": (20_001, 4, 1.0, (1, 3)),    # shard head bits, uneven shards
    "d18": (10_623, 18, 1.0, None),          # only the leading 16 coordinates enter the key
}
BLOCK_SHAPES = ("d4", "d6", "d8_sampled")
_CASES = {}


def case(name):
    """One cloud, its oracle embedding and the library's lattice, built once for the module."""
    if name not in _CASES:
        import simplex_gp_amd as plx
        from simplex_gp_amd import _native as nv
        n, d, ell, shard = SHAPES[name]
        g = torch.Generator().manual_seed(1234)
        x = (torch.randn(n, d, generator=g) / ell).contiguous()
        oracle.set_exact_mode(False)
        try:
            o = oracle.Lattice(x.numpy(), RBF1)
            greedy, entry_vertex = o.greedy, o.entry_vertex
            o.close()
        finally:
            oracle.set_exact_mode(True)
        nv.check(nv.lib().plx_tune(b"block_e", 24), "plx_tune")
        try:
            lat = plx.Lattice().build(x.cuda(), RBF1, shard=shard)
            if name in BLOCK_SHAPES:
                lat.prepare(1)
        finally:
            nv.check(nv.lib().plx_tune(b"block_e", 0), "plx_tune")
        _CASES[name] = dict(x=x.numpy(), greedy=greedy, entry_vertex=entry_vertex, lat=lat,
                            perm=lat.shard_perm().cpu().numpy(), shard=shard)
    return _CASES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_order_is_a_stable_sort_of_the_cell_key(name):
    c = case(name)
    n = c["x"].shape[0]
    index, count = c["shard"] or (0, 1)
    key = order_keys(fixed_cells(c["greedy"]), count)
    base, extra = divmod(n, count)
    begin = index * base + min(index, extra)
    n_own = base + (1 if index < extra else 0)
    perm = c["perm"]
    # the shard's rows, each once: the shard id leads the key, so they fill the shard's own index range
    assert perm.shape == (n_own,) and np.array_equal(np.sort(perm), np.arange(n_own))
    k = key[perm + begin]
    step = k[1:].astype(np.int64) - k[:-1].astype(np.int64)           # (keys have at most 62 bits)
    unsorted = np.flatnonzero(step < 0)
    unstable = np.flatnonzero((step == 0) & (perm[1:] < perm[:-1]))
    print(f"{name}: n {n}, distinct keys {len(np.unique(k))}, descents {len(unsorted)}, ties out of caller order {len(unstable)}")
    assert len(unsorted) == 0, f"key decreases at sorted positions {unsorted[:8]}"
    assert len(unstable) == 0, f"equal keys out of caller order at sorted positions {unstable[:8]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", BLOCK_SHAPES)
def test_block_rows_match_the_model_and_beat_the_rounded_key(name):
    """Block rows of the library (block_e = 24) = distinct (block, vertex) pairs of the model under the library's own order,
    and fewer than under the rounded key.  Measured: 5,434 / 57,717 / 64,626 against 7,205 / 69,337 / 72,306 (the library's
    counts under the rounded key were the same three numbers: profiles/order_cell_measured.md)."""
    c = case(name)
    n, d = c["x"].shape
    P = block_points(24, d + 1)
    want = count_block_rows(c["perm"], c["entry_vertex"], P)
    rounded_perm = np.argsort(order_keys(rounded_cells(c["x"], RBF1)), kind="stable")
    rounded = count_block_rows(rounded_perm, c["entry_vertex"], P)
    got = c["lat"].block_rows
    print(f"{name}: P {P}, block rows {got}, model under the library's order {want}, model under the rounded key {rounded}")
    assert got == want
    assert got < rounded
