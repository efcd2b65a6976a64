"""The one-sided float64 position gradient of the rectangular product (plx_backward_splat_rows_f64 /
plx_backward_contract_rows_f64 / plx_apply_backward_rows_f64, simplex_gp_amd/csrc/plx_rows_backward_f64.hip) on the GPU.

Yardstick: tests/rows_backward64.one_sided -- the half stack [ a | a (x) x ] of the rows of a, zero-padded over the N = 701
stacked points, filtered in float64 by Lattice64 on the derivative-tap lattice of x rounded to float32, the contraction
against b redone in np.longdouble.  x is NOT representable in float32 (positions64), so a stack formed from the rounded
copy shows.  The ranges are those of tests.test_rows_fp64.ranges: the "source" side is the a range, the "output" side the
b range of a case's call.

Bits (torch.equal, -0.0 equal to +0.0), on every case: (a) the stack splat against Lattice.splat_rows of the explicit half
stack, all stride columns; (b) filtered against columns [0, L) of Lattice.apply_rows of it; (c) filtered against the rows of
grad_src of Lattice.apply_backward on the zero-padded n-row matrices; (d) staged against fused; (e) two calls, device_bytes
on the second, d_filtered = NULL.

The bar, per entry of grad_x, none left out, with U = 2^-52 and k = depth(lat):
    |got - want| <= 2 (k + 2 (L + 1)) U T''[i, k],   T'' = 2 sum_l ( |b_l x_k| t(a)_l + |b_l| t(a (x) x)_lk ),  t(.) = terms64
Every filtered entry carries at most k roundings of its own terms (the stack multiply is one of them), the contraction adds
two multiplies and 2 L additions, the factor 2 covers the float64 reference filter, which obeys the same bound: the
structure of tests/test_backward_f64_gpu.py with half as many terms.  Where T'' = 0 the entry must be exactly 0.  filtered
per entry: k U terms64(a).

Against the padded call: the two one-sided results (the case's call and the one with a and b swapped) added into [n][d]
agree with grad_x of Lattice.apply_backward(A, B, x) within twice the square bar, 2 * 2 (k + 4 (L + 1)) U T'.  Whether they
were in fact equal is printed, not asserted.  Worst ratios per kernel family are printed at the end (pytest -s) and copied
to profiles/rows_backward_f64_measured.md.
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
from tests.gpubuf import SENTINEL, Buf, check_buffers
from tests.lattice64 import Lattice64
from tests.rows_backward64 import CASES, IDS, LD, U, chunks, half_stack64, one_sided, scatter_sides
from tests.test_backward_f64_gpu import cuda, depth, dkernel, positions64, ptr, ratio_to_bar, reference, stream_ptr
from tests.test_rows_fp64 import ranges

pytestmark = pytest.mark.gpu

N = 701
PLX_ERR_INVALID, PLX_ERR_STATE, PLX_ERR_TOO_LARGE = 1, 5, 6
F64 = torch.float64
CHUNK = ("rows64_backward_splat_chunk_kernel", "rows64_backward_contract_chunk_kernel")
WIDE = ("rows64_backward_splat_wide_kernel", "rows64_backward_contract_wide_kernel")

_REF = {}
WORST = {}            # family -> [grad_x ratio to its bar, filtered ratio to its bar, sides / padded ratio, cases]
EQUAL_TO_PADDED = {}  # case id -> whether the scattered sides were bit-equal to the padded gradient (printed, not asserted)
REACHED = set()


def expect(d, L):
    return CHUNK if chunks(d, L) <= 64 else WIDE


def stride_of(d, L):
    return 2 * chunks(d, L)


def raw_splat(lat, a, ab, ac, x, L, values, stream=None):
    return nv.lib().plx_backward_splat_rows_f64(lat._h, a, ab, ac, x, L, values, stream or stream_ptr())


def raw_contract(lat, values, b, bb, bc, x, L, gx, fl, stream=None):
    return nv.lib().plx_backward_contract_rows_f64(lat._h, values, b, bb, bc, x, L, gx, fl, stream or stream_ptr())


def raw_apply(lat, a, ab, ac, b, bb, bc, x, L, gx, fl, stream=None):
    return nv.lib().plx_apply_backward_rows_f64(lat._h, a, ab, ac, b, bb, bc, x, L, gx, fl, stream or stream_ptr())


def family_of(lat):
    k = lat.rows_f64_kernels()
    return ("+".join(k["splat"]), "+".join(k["slice"]))


def padded(rows, rng_, n):
    out = np.zeros((n, rows.shape[1]))
    out[rng_[0]:rng_[0] + rng_[1]] = rows
    return out


def case_data(idx):
    """Everything a case needs, built once for the module: inputs, the yardsticks, the GPU lattice."""
    if idx not in _REF:
        d, L, order, profile, kind, aligned, rname = CASES[idx]
        dtaps = dkernel(profile, order).get_deriv_coeffs().numpy()
        x = positions64(kind, N, d, seed=idx + 1, coeffs=dtaps)
        a_rng, b_rng = ranges(rname, N)
        rng = np.random.default_rng(2000 + idx)
        a, b = rng.standard_normal((a_rng[1], L)), rng.standard_normal((b_rng[1], L))
        if kind == "isolated":
            a[::2] = 0.0                               # rows no term reaches: T'' = 0 there, and so must the gradient be
            b[::2] = 0.0
        l64 = Lattice64(x, dtaps)
        lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
        assert lat.m == l64.m and lat.order == order
        side = one_sided(a, a_rng, b, b_rng, x, l64)
        square = reference(padded(a, a_rng, N), padded(b, b_rng, N), x, l64)     # G = a on its rows, S = b on its rows
        _REF[idx] = (a, b, x, a_rng, b_rng, side, square, lat)
    return _REF[idx]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_rows_backward_f64_against_lattice64(idx):
    d, L, order, profile, kind, aligned, rname = CASES[idx]
    a, b, x, (ab, ac), (bb, bc), (want, want_f, T, ta), (sq_want, _, sq_T, _), lat = case_data(idx)
    H, stride, off, label = L * (1 + d), stride_of(d, L), 0 if aligned else 1, IDS[idx]
    ba, bbuf, bx = (Buf(t, offset=off, dtype=F64) for t in (a, b, x))
    new_out = lambda rows, cols: Buf(count=rows * cols, offset=off, dtype=F64, fill=SENTINEL)      # noqa: E731
    gx, fl = new_out(bc, d), new_out(bc, L)
    assert ba.ptr.value % 16 == (0 if aligned else 8)
    # the fused call; (e) two calls bit-equal; the second call of a (range pair, width) leaves plx_device_bytes alone
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == 0, nv.lib().plx_last_error()
    fam = family_of(lat)
    assert fam == expect(d, L), (label, fam)
    assert lat.f64_kernels()["blur_axis"] == ["f64_blur_chunk_kernel"]
    REACHED.update(fam)
    got_x, got_f = gx.cpu(bc, d).clone(), fl.cpu(bc, L).clone()
    bytes1 = lat.device_bytes
    gx2, fl2 = new_out(bc, d), new_out(bc, L)
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx2.ptr, fl2.ptr) == 0
    assert lat.device_bytes == bytes1, (label, "the second call of a range pair moved plx_device_bytes")
    assert torch.equal(gx2.cpu(bc, d), got_x) and torch.equal(fl2.cpu(bc, L), got_f), (label, "not deterministic")
    gx3 = new_out(bc, d)
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx3.ptr, None) == 0       # d_filtered = NULL
    assert torch.equal(gx3.cpu(bc, d), got_x)
    # (a) the stack splat against splat_rows of the explicit half stack, one multiply per product element, all columns
    ta_, tx_ = ba.view.view(ac, L), bx.view.view(N, d)[ab:ab + ac]
    hs = torch.cat([ta_, (ta_[:, :, None] * tx_[:, None, :]).reshape(ac, L * d)], dim=1).contiguous()
    assert hs.shape == (ac, H) and np.array_equal(hs.cpu().numpy(), half_stack64(a, x[ab:ab + ac]))
    values = Buf(count=lat.m * stride, dtype=F64, fill=SENTINEL)
    assert raw_splat(lat, ba.ptr, ab, ac, bx.ptr, L, values.ptr) == 0, nv.lib().plx_last_error()
    explicit = lat.splat_rows(hs, ab)
    assert explicit.shape == (lat.m, stride)
    assert torch.equal(values.view.view(lat.m, stride), explicit), (label, "stack splat differs from splat_rows(half stack)")
    # (b) filtered against columns [0, L) of apply_rows(half stack)
    assert torch.equal(got_f, lat.apply_rows(hs, ab, bb, bc)[:, :L].cpu()), (label, "filtered differs from apply_rows")
    # (d) staged against fused
    assert raw_splat(lat, ba.ptr, ab, ac, bx.ptr, L, values.ptr) == 0
    blurred = lat.blur(values.view.view(lat.m, stride), vd=H)
    gx4, fl4 = new_out(bc, d), new_out(bc, L)
    assert raw_contract(lat, ptr(blurred), bbuf.ptr, bb, bc, bx.ptr, L, gx4.ptr, fl4.ptr) == 0, nv.lib().plx_last_error()
    assert family_of(lat) == fam
    assert torch.equal(gx4.cpu(bc, d), got_x) and torch.equal(fl4.cpu(bc, L), got_f), (label, "staged differs from fused")
    # the other side: a and b swapped, for the comparison with the padded call
    gx5 = new_out(ac, d)
    assert raw_apply(lat, bbuf.ptr, bb, bc, ba.ptr, ab, ac, bx.ptr, L, gx5.ptr, None) == 0, nv.lib().plx_last_error()
    assert family_of(lat) == fam
    other_x = gx5.cpu(ac, d).clone()
    check_buffers(inputs=(ba, bbuf, bx), outputs=(gx, fl, gx2, fl2, gx3, gx4, fl4, gx5, values))
    # (c) filtered against the rows of grad_src of the padded square call; the scattered sides against its grad_x
    A, B = cuda(padded(a, (ab, ac), N)), cuda(padded(b, (bb, bc), N))
    pad_x, pad_s = lat.apply_backward(A, B, bx.view.view(N, d))
    assert torch.equal(got_f, pad_s[bb:bb + bc].cpu()), (label, "filtered differs from the padded grad_src rows")
    k = depth(lat)
    sides = scatter_sides(N, d, (bb, bc), (ab, ac), got_x.numpy(), other_x.numpy())
    pad_x = pad_x.cpu().numpy()
    rp = ratio_to_bar(sides, pad_x.astype(LD), sq_T, 2 * 2 * (k + 4 * (L + 1)) * U, label)
    EQUAL_TO_PADDED[label] = bool(np.array_equal(sides, pad_x))
    # the bar: every entry of grad_x; filtered against the bar of the product
    bar_x, bar_f = 2 * (k + 2 * (L + 1)) * U, k * U
    rx = ratio_to_bar(got_x.numpy(), want, T, bar_x, label)
    rf = ratio_to_bar(got_f.numpy(), want_f.astype(LD), ta, bar_f, label)
    w = WORST.setdefault(fam, [0.0, 0.0, 0.0, 0])
    w[0], w[1], w[2], w[3] = max(w[0], rx), max(w[1], rf), max(w[2], rp), w[3] + 1
    print(f"{label}: k = {k}  grad_x / bar {rx:.3f} (bar {bar_x:.2e} T'')  filtered / bar {rf:.3f} (bar {bar_f:.2e} T)  "
          f"sides / (2 square bar) {rp:.3f}  equal to padded: {EQUAL_TO_PADDED[label]}  {fam}")
    assert rx <= 1.0, (label, "grad_x entry ratio to the bar", rx)
    assert rf <= 1.0, (label, "filtered entry ratio to the bar", rf)
    assert rp <= 1.0, (label, "the two sides against the padded gradient, ratio to twice the square bar", rp)
    if kind == "isolated":
        zero = (T == 0).all(axis=1)
        assert zero.sum() >= bc // 2 and bool((got_x.numpy()[zero] == 0).all()), label
        assert float(np.abs(got_x.numpy()).max()) <= bar_x * float(T.max()), (label, "the true gradient vanishes")


def test_column_limit_edge():
    """stride = 2048 exactly (d = 7, L = 256: 1024 chunks, 64 KiB of LDS per workgroup), the widest row the contraction
    holds.  grad_x is judged against the contraction in np.longdouble of the DEVICE's own filtered half stack, which the
    kernel's on-chip row equals bit for bit: what is left is the contraction alone, a recursive sum of 2 L products of at
    most three roundings each, so |got - want| <= (2 L + 4) 2^-53 T with T twice the sum of the absolute terms."""
    d, L = 7, 256
    H = L * (1 + d)
    assert H == plx.Lattice.BACKWARD_ROWS_F64_MAX_STRIDE and plx.Lattice.backward_rows_f64_ok(L, d)
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    x = positions64("gauss1", N, d, seed=78, coeffs=dtaps)
    (ab, ac), (bb, bc) = ranges("head0.5", N)
    rng = np.random.default_rng(78)
    a, b = rng.standard_normal((ac, L)), rng.standard_normal((bc, L))
    lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
    ba, bbuf, bx = (Buf(t, offset=1, dtype=F64) for t in (a, b, x))
    gx, fl = Buf(count=bc * d, offset=1, dtype=F64, fill=SENTINEL), Buf(count=bc * L, offset=1, dtype=F64, fill=SENTINEL)
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == 0, nv.lib().plx_last_error()
    assert family_of(lat) == WIDE
    REACHED.update(WIDE)
    hs = cuda(half_stack64(a, x[ab:ab + ac]))
    values = Buf(count=lat.m * H, dtype=F64, fill=SENTINEL)
    assert raw_splat(lat, ba.ptr, ab, ac, bx.ptr, L, values.ptr) == 0
    assert torch.equal(values.view.view(lat.m, H), lat.splat_rows(hs, ab))
    f = lat.apply_rows(hs, ab, bb, bc).cpu().numpy()
    assert np.array_equal(fl.np(bc, L), f[:, :L])
    check_buffers(inputs=(ba, bbuf, bx), outputs=(gx, fl, values))
    wa, wax = f[:, :L].astype(LD), f[:, L:].astype(LD).reshape(bc, L, d)
    b3, x3 = b.astype(LD)[:, :, None], x[bb:bb + bc].astype(LD)[:, None, :]
    t1, t2 = b3 * x3 * wa[:, :, None], b3 * wax
    want = -2 * (t1 - t2).sum(1)
    T = (2 * (np.abs(t1) + np.abs(t2)).sum(1)).astype(np.float64)
    r = ratio_to_bar(gx.np(bc, d), want, T, (2 * L + 4) * 2.0 ** -53, "limit")
    print(f"column limit d={d} L={L}: grad_x against the contraction of the device's filtered half stack / bar {r:.3f}")
    assert r <= 1.0, r
    lat.close()


def test_refusals_leave_the_outputs_untouched():
    d, L = 3, 2
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, d))
    (ab, ac), (bb, bc) = ranges("head0.8", N)
    ba, bbuf = Buf(rng.standard_normal((ac, L)), dtype=F64), Buf(rng.standard_normal((bc, L)), dtype=F64)
    bx = Buf(x, dtype=F64)
    gx, fl = Buf(count=bc * d, dtype=F64, fill=SENTINEL), Buf(count=bc * L, dtype=F64, fill=SENTINEL)
    err = nv.lib().plx_last_error

    def all_three(lat, values, nrhs=L, a=ba, b=bbuf, a_rng=(ab, ac), b_rng=(bb, bc), out_f=fl):
        return (raw_splat(lat, a.ptr, a_rng[0], a_rng[1], bx.ptr, nrhs, values.ptr),
                raw_contract(lat, values.ptr, b.ptr, b_rng[0], b_rng[1], bx.ptr, nrhs, gx.ptr, out_f.ptr),
                raw_apply(lat, a.ptr, a_rng[0], a_rng[1], b.ptr, b_rng[0], b_rng[1], bx.ptr, nrhs, gx.ptr, out_f.ptr))

    def untouched(*more):
        torch.cuda.synchronize()
        assert all(t.unchanged() for t in (gx, fl) + more), "a refused call wrote an output"
        check_buffers(inputs=(ba, bbuf, bx), outputs=(gx, fl) + more)

    # a lattice that is not built
    lat = plx.Lattice()
    values = Buf(count=4096, dtype=F64, fill=SENTINEL)
    bytes0 = lat.device_bytes
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"not built" in err()
    assert lat.device_bytes == bytes0
    untouched(values)
    # one shard of two
    lat.build(cuda(x, np.float32), dtaps, shard=(0, 2))
    bytes0 = lat.device_bytes
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"shard" in err()
    assert lat.device_bytes == bytes0
    untouched(values)
    lat.close()
    # a build that replayed the reference's table growth
    nv.check(nv.lib().plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
    finally:
        nv.check(nv.lib().plx_tune(b"reference_growth", 0), "plx_tune")
    assert lat.reference_growth_info()["replayed"]
    bytes0 = lat.device_bytes
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"reference_growth" in err()
    assert lat.device_bytes == bytes0
    with pytest.raises(PlxError) as e:
        lat.apply_backward_rows(ba.view.view(ac, L), ab, bbuf.view.view(bc, L), bb, bx.view.view(N, d))
    assert e.value.code == PLX_ERR_STATE
    untouched(values)
    lat.close()
    # on a plain build: d_values off 16-byte alignment
    lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
    bytes0 = lat.device_bytes
    stride = stride_of(d, L)
    values = Buf(count=lat.m * stride, offset=1, dtype=F64, fill=SENTINEL)
    assert values.ptr.value % 16 == 8
    assert raw_splat(lat, ba.ptr, ab, ac, bx.ptr, L, values.ptr) == PLX_ERR_INVALID and b"16-byte" in err()
    assert raw_contract(lat, values.ptr, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"16-byte" in err()
    untouched(values)
    # a range past n, a negative begin, a count < 1 -- on either side
    values = Buf(count=lat.m * stride, dtype=F64, fill=SENTINEL)
    for bad in ((N - 3, 4), (-1, 4), (0, N + 1), (0, 0)):
        # only the calls that take the bad range: the third would be a valid call, and run
        assert raw_splat(lat, ba.ptr, bad[0], bad[1], bx.ptr, L, values.ptr) == PLX_ERR_INVALID, bad
        assert raw_apply(lat, ba.ptr, bad[0], bad[1], bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID, bad
        assert raw_contract(lat, values.ptr, bbuf.ptr, bad[0], bad[1], bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID, bad
        assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bad[0], bad[1], bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID, bad
    assert raw_splat(lat, ba.ptr, N - 3, 4, bx.ptr, L, values.ptr) == PLX_ERR_INVALID and b"range" in err()
    with pytest.raises(ValueError, match="range"):
        lat.apply_backward_rows(ba.view.view(ac, L), N - 3, bbuf.view.view(bc, L), bb, bx.view.view(N, d))
    # the lattice-free refusals once more, next to a real lattice
    assert all_three(lat, values, nrhs=0) == (PLX_ERR_INVALID,) * 3 and b"positive" in err()
    assert raw_apply(lat, None, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, None, fl.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, ctypes.c_void_p(bx.ptr.value + 4), L, gx.ptr,
                     fl.ptr) == PLX_ERR_INVALID and b"8-byte" in err()
    assert raw_apply(lat, gx.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, gx.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_contract(lat, values.ptr, bbuf.ptr, bb, bc, bx.ptr, L, values.ptr, None) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_splat(lat, ba.ptr, ab, ac, values.ptr, L, values.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert lat.device_bytes == bytes0
    untouched(values)
    lat.close()
    # the column limit: 257 * 8 = 2056 > 2048 (buffers of the full size: nothing could run past them)
    d7 = 7
    assert not plx.Lattice.backward_rows_f64_ok(257, d7) and plx.Lattice.backward_rows_f64_ok(256, d7)
    x7 = Buf(rng.standard_normal((N, d7)), dtype=F64)
    lat = plx.Lattice().build(x7.view.view(N, d7).float(), dtaps)
    wide = Buf(count=N * 257, dtype=F64, fill=0.5)
    gx7, fl_w = Buf(count=N * d7, dtype=F64, fill=SENTINEL), Buf(count=N * 257, dtype=F64, fill=SENTINEL)
    values = Buf(count=lat.m * 2056, dtype=F64, fill=SENTINEL)
    bytes0 = lat.device_bytes
    full = (0, N)
    assert raw_splat(lat, wide.ptr, *full, x7.ptr, 257, values.ptr) == PLX_ERR_INVALID and b"2048" in err()
    assert raw_contract(lat, values.ptr, wide.ptr, *full, x7.ptr, 257, gx7.ptr, fl_w.ptr) == PLX_ERR_INVALID and b"2048" in err()
    assert raw_apply(lat, wide.ptr, *full, wide.ptr, *full, x7.ptr, 257, gx7.ptr, fl_w.ptr) == PLX_ERR_INVALID
    assert b"2048" in err()
    with pytest.raises(PlxError) as e:
        lat.apply_backward_rows(wide.view.view(N, 257), 0, wide.view.view(N, 257), 0, x7.view.view(N, d7))
    assert e.value.code == PLX_ERR_INVALID and "2048" in str(e.value)
    assert lat.device_bytes == bytes0
    torch.cuda.synchronize()
    assert gx7.unchanged() and fl_w.unchanged() and values.unchanged()
    check_buffers(inputs=(wide, x7), outputs=(gx7, fl_w, values))
    lat.close()


def test_too_large_is_refused_before_any_work():
    """a_count * stride = 2^31 exactly: n = 2^20 points on a line (d = 1), 1024 columns, stride 2048.  a and b are one
    uninitialised allocation of the full n x 1024 size, so that nothing could be read past its end; no output may be
    written."""
    n, d, L = 1 << 20, 1, 1024
    assert plx.Lattice.backward_rows_f64_ok(L, d)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(1), dtype=F64).cuda()
    lat = plx.Lattice().build(x.float(), dkernel("rbf", 1).get_deriv_coeffs().numpy())
    big = torch.empty((n, L), dtype=F64, device="cuda")
    gx = Buf(count=n * d, dtype=F64, fill=SENTINEL)
    values = Buf(count=64, dtype=F64, fill=SENTINEL)
    bytes0 = lat.device_bytes
    assert raw_apply(lat, ptr(big), 0, n, ptr(big), 0, n, ptr(x), L, gx.ptr, None) == PLX_ERR_TOO_LARGE
    assert b"2^31" in nv.lib().plx_last_error()
    assert raw_splat(lat, ptr(big), 0, n, ptr(x), L, values.ptr) == PLX_ERR_TOO_LARGE
    assert raw_contract(lat, values.ptr, ptr(big), 0, n, ptr(x), L, gx.ptr, None) == PLX_ERR_TOO_LARGE
    torch.cuda.synchronize()
    assert lat.device_bytes == bytes0 and gx.unchanged() and values.unchanged()
    check_buffers(outputs=(gx, values))
    lat.close()


def test_capture():
    d, L = 4, 3
    n = 5000
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    rng = np.random.default_rng(9)
    (ab, ac), (bb, bc) = ranges("head0.8", n)
    x = cuda(rng.standard_normal((n, d)))
    a, b = cuda(rng.standard_normal((ac, L))), cuda(rng.standard_normal((bc, L)))
    lat = plx.Lattice().build(x.float(), dtaps)
    gx, fl = torch.full((bc, d), SENTINEL, dtype=F64, device="cuda"), torch.full((bc, L), SENTINEL, dtype=F64, device="cuda")
    bytes0 = lat.device_bytes
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    # the first call of a (range pair, width) under capture is refused, and nothing is written
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        rc = raw_apply(lat, ptr(a), ab, ac, ptr(b), bb, bc, ptr(x), L, ptr(gx), ptr(fl))
    assert rc == PLX_ERR_STATE and b"captured" in nv.lib().plx_last_error()
    del graph
    torch.cuda.synchronize()
    assert lat.device_bytes == bytes0
    assert bool((gx == SENTINEL).all()) and bool((fl == SENTINEL).all())
    with torch.cuda.stream(st):
        eager_x, eager_f = lat.apply_backward_rows(a, ab, b, bb, x)       # the warm-up: tables and workspace
        first = lat.device_bytes
        assert first > bytes0
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            rc = raw_apply(lat, ptr(a), ab, ac, ptr(b), bb, bc, ptr(x), L, ptr(gx), ptr(fl))
        assert rc == 0, nv.lib().plx_last_error()
        graph.replay()
        st.synchronize()
        assert torch.equal(gx, eager_x) and torch.equal(fl, eager_f)
        # ... also on new inputs copied into place
        a2, b2 = cuda(rng.standard_normal((ac, L))), cuda(rng.standard_normal((bc, L)))
        want_x, want_f = lat.apply_backward_rows(a2, ab, b2, bb, x)
        a.copy_(a2)
        b.copy_(b2)
        graph.replay()
        st.synchronize()
        assert torch.equal(gx, want_x) and torch.equal(fl, want_f)
        assert not torch.equal(want_x, eager_x)
        assert lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


N_IN, N_OUT = 140, 561


def _cached_rows_kernels():
    names = set()
    for lat, _, _ in plx.lattice_cache()._entries.values():
        fam = lat.rows_f64_kernels()
        names.update(fam["splat"] + fam["slice"])
    return names


def _operator_grads(dk, xin, xout, v, w, native, transposed):
    """(out, xin.grad, xout.grad, V.grad, rows kernels seen on the cached lattices) of (K V . W).sum().backward() for
    K = RectangularLazyLattice(xin, xout) or, transposed, its _transpose_nonbatch() (V then lives on xin)."""
    plx.RectangularLazyLattice.native_rows_grad_f64 = native
    plx.lattice_cache().clear()
    ti, to, tv = cuda(xin).requires_grad_(True), cuda(xout).requires_grad_(True), cuda(v).requires_grad_(True)
    op = plx.RectangularLazyLattice(ti, to, dk)
    if transposed:
        op = op._transpose_nonbatch()
    out = op._matmul(tv)
    (out * cuda(w)).sum().backward()
    names = _cached_rows_kernels()
    return out.detach().cpu(), ti.grad.cpu().numpy(), to.grad.cpu().numpy(), tv.grad.cpu().numpy(), names


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("d,L", [(3, 2), (8, 1), (8, 11)])
def test_autograd_in_double_both_routes(d, L, transposed):
    """(K(xin, xout) V . W).sum().backward() in double with native_rows_grad_f64 on and off: the outputs are torch.equal;
    xin.grad and xout.grad of each route are under the square bar 2 (k + 4 (L + 1)) U T' against the reference of the
    padded problem on the stacked points [xout; xin]; the two routes agree within twice that bar; V.grad is under
    k U terms64; the native route launched the new kernels and the padded one did not.  transposed: the same through
    _transpose_nonbatch(), the roles of the two point sets swapped."""
    dk = dkernel("rbf", 1)
    dtaps = dk.get_deriv_coeffs().numpy()
    x = positions64("gauss1", N, d, seed=3 * d + L, coeffs=dtaps)           # the stacked points [xout; xin]
    xout, xin = x[:N_OUT], x[N_OUT:]
    rng = np.random.default_rng(10 * d + L)
    src_rng, out_rng = ((N_OUT, N_IN), (0, N_OUT)) if transposed else ((0, N_OUT), (N_OUT, N_IN))
    v, w = rng.standard_normal((src_rng[1], L)), rng.standard_normal((out_rng[1], L))
    l64 = Lattice64(x, dtaps)
    want, want_gs, T, tg = reference(padded(w, out_rng, N), padded(v, src_rng, N), x, l64)
    lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
    k = depth(lat)
    lat.close()
    before = plx.RectangularLazyLattice.native_rows_grad_f64
    res = {}
    try:
        for native in (True, False):
            res[native] = _operator_grads(dk, xin, xout, v, w, native, transposed)
    finally:
        plx.RectangularLazyLattice.native_rows_grad_f64 = before
        plx.lattice_cache().clear()
    assert set(expect(d, L)) <= res[True][4], res[True][4]                   # the native route ran the new kernels ...
    assert not set(CHUNK + WIDE) & res[False][4], res[False][4]              # ... and the padded route did not
    REACHED.update(res[True][4] & set(CHUNK + WIDE))
    assert res[True][0].shape == (out_rng[1], L) and torch.equal(res[True][0], res[False][0])
    bar_x, bar_s = 2 * (k + 4 * (L + 1)) * U, k * U
    s0, s1 = src_rng[0], src_rng[0] + src_rng[1]
    grads = {}
    for native, (_, gin, gout, gv, _) in res.items():
        grads[native] = np.concatenate([gout, gin])                          # rows of the stacked points
        rx = ratio_to_bar(grads[native], want, T, bar_x, "positions.grad")
        rs = ratio_to_bar(gv, want_gs[s0:s1].astype(LD), tg[s0:s1], bar_s, "V.grad")
        print(f"autograd double d={d} L={L} transposed={transposed} native={native}: x.grad / bar {rx:.3f}  "
              f"V.grad / bar {rs:.3f}")
        assert rx <= 1.0 and rs <= 1.0, (native, rx, rs)
        assert gin.dtype == np.float64 and gout.dtype == np.float64 and gv.dtype == np.float64
    agree = ratio_to_bar(grads[True], grads[False].astype(LD), T, 2 * bar_x, "routes")
    print(f"autograd double d={d} L={L} transposed={transposed}: native against padded route, x.grad / (2 bar) {agree:.3f}")
    assert agree <= 1.0, agree


def family_report():
    lines = ["one-sided float64 position gradient against Lattice64, worst ratio to the bar per kernel family "
             "(grad_x, filtered, two sides against the padded call / twice the square bar):"]
    for fam, (a, b, c, cases) in sorted(WORST.items()):
        lines.append(f"  {fam[0]} | {fam[1]}: {a:.3f} {b:.3f} {c:.3f} ({cases} cases)")
    lines.append("two sides bit-equal to the padded gradient: "
                 + ", ".join(f"{label}: {'yes' if eq else 'no'}" for label, eq in EQUAL_TO_PADDED.items()))
    return "\n".join(lines)


def test_every_new_kernel_was_launched():
    """Every kernel name plx_rows_backward_f64.hip can report ran in this module (run as a whole)."""
    print(family_report())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "simplex_gp_amd", "csrc", "plx_rows_backward_f64.hip")).read()
    literals = set()
    for stmt in re.finditer(r"\bk(?:Splat|Contract)(?:Chunk|Wide)\s*=([^;]*);", text):
        literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    assert literals == set(CHUNK + WIDE), literals
    assert REACHED == literals, sorted(literals - REACHED)
    for lat in (v[-1] for v in _REF.values()):
        lat.close()
    _REF.clear()
