"""The one-sided fp32 position gradient of the rectangular product (plx_backward_splat_rows / plx_backward_contract_rows /
plx_apply_backward_rows, simplex_gp_amd/csrc/plx_rows_backward.hip) on the GPU.

Yardstick: tests/rows_backward64.one_sided -- the half stack [ a | a (x) x ] of the rows of a, zero-padded over the N = 701
stacked points, filtered in float64 by Lattice64 on the derivative-tap lattice, the contraction against b redone in
np.longdouble.  a, b and x are float32 values; the same values, widened, go to Lattice64.  The ranges are those of
tests.test_rows_fp64.ranges: the "source" side is the a range, the "output" side the b range of a case's call.

Bits (torch.equal, -0.0 equal to +0.0), on every case: (a) the stack splat against Lattice.splat_rows of the explicit float32
half stack (one multiply per product element), all stride columns; (b) filtered against columns [0, L) of Lattice.apply_rows of
it; (c) staged (splat, Lattice.blur at vd = H, contract) against fused; (d) two fused calls, device_bytes unmoved by the
second; (e) d_filtered = NULL; (f) sentinel-filled buffers untouched outside the outputs.

The bar, per entry of grad_x, none left out, with k32 = tests/rows_backward32.k32 (derived there and in DESIGN.md section 22):
    |got - want| <= (k32 + 2 (L + 1)) 2^-23 T''[i, k],   T'' = 2 sum_l ( |b_l x_k| t(a)_l + |b_l| t(a (x) x)_lk ),  t(.) = terms64
Every filtered entry carries at most k32 roundings of its own terms, the contraction adds two multiplies and 2 L additions.
Where T'' = 0 the entry must be exactly 0.  filtered per entry: k32 2^-23 terms64(a).

Against the padded problem: the two one-sided results (the case's call and the one with a and b swapped) added into [n][d]
agree with the float64 square reference (tests/test_backward_f64_gpu.reference on the zero-padded matrices) within
2 (k32 + 4 (L + 1)) 2^-23 T'; where backward_fusable(L, d), Lattice.apply_backward on the padded matrices is held to the same
bar.  Worst ratios per kernel family are printed at the end (pytest -s) and copied to profiles/rows_backward_measured.md.
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
from tests.lattice64 import Lattice64, cloud, rel_l2
from tests.rows_backward32 import CASES, IDS, U32, chunks32, half_stack64, k32, one_sided, scatter_sides
from tests.test_backward_f64_gpu import dkernel, ptr, ratio_to_bar, reference, stream_ptr
from tests.test_backward_fp64 import REL
from tests.test_rows_fp64 import ranges

pytestmark = pytest.mark.gpu

N = 701
LD = np.longdouble
PLX_ERR_INVALID, PLX_ERR_STATE, PLX_ERR_TOO_LARGE = 1, 5, 6
F32 = torch.float32
CHUNK = ("rows_backward_splat_chunk_kernel", "rows_backward_contract_chunk_kernel")
WIDE = ("rows_backward_splat_wide_kernel", "rows_backward_contract_wide_kernel")

_REF = {}
WORST = {}            # family -> [grad_x ratio to its bar, filtered ratio to its bar, sides / square bar, cases]
REACHED = set()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def f32_values(rng, shape):
    """Standard normal float32 values, as float64."""
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def expect(d, L):
    return CHUNK if chunks32(d, L) <= 64 else WIDE


def stride_of(d, L):
    return 4 * chunks32(d, L)


def raw_splat(lat, a, ab, ac, x, L, values, stream=None):
    return nv.lib().plx_backward_splat_rows(lat._h, a, ab, ac, x, L, values, stream or stream_ptr())


def raw_contract(lat, values, b, bb, bc, x, L, gx, fl, stream=None):
    return nv.lib().plx_backward_contract_rows(lat._h, values, b, bb, bc, x, L, gx, fl, stream or stream_ptr())


def raw_apply(lat, a, ab, ac, b, bb, bc, x, L, gx, fl, stream=None):
    return nv.lib().plx_apply_backward_rows(lat._h, a, ab, ac, b, bb, bc, x, L, gx, fl, stream or stream_ptr())


def family_of(lat):
    k = lat.rows_kernels()
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
        x32 = cloud(kind, N, d, seed=idx + 1, coeffs=dtaps)
        assert x32.dtype == np.float32
        x = x32.astype(np.float64)
        a_rng, b_rng = ranges(rname, N)
        rng = np.random.default_rng(3000 + idx)
        a, b = f32_values(rng, (a_rng[1], L)), f32_values(rng, (b_rng[1], L))
        if kind == "isolated":
            a[::2] = 0.0                               # rows no term reaches: T'' = 0 there, and so must the gradient be
            b[::2] = 0.0
        l64 = Lattice64(x, dtaps)
        lat = plx.Lattice().build(cuda(x), dtaps)
        assert lat.m == l64.m and lat.order == order
        side = one_sided(a, a_rng, b, b_rng, x, l64)
        square = reference(padded(a, a_rng, N), padded(b, b_rng, N), x, l64)     # G = a on its rows, S = b on its rows
        _REF[idx] = (a, b, x, a_rng, b_rng, side, square, k32(l64), lat)
    return _REF[idx]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_rows_backward_against_lattice64(idx):
    d, L, order, profile, kind, aligned, rname = CASES[idx]
    a, b, x, (ab, ac), (bb, bc), (want, want_f, T, ta), (sq_want, _, sq_T, _), k, lat = case_data(idx)
    H, stride, off, label = L * (1 + d), stride_of(d, L), 0 if aligned else 1, IDS[idx]
    ba, bbuf, bx = (Buf(t, offset=off, dtype=F32) for t in (a, b, x))
    new_out = lambda rows, cols: Buf(count=rows * cols, offset=off, dtype=F32, fill=SENTINEL)      # noqa: E731
    gx, fl = new_out(bc, d), new_out(bc, L)
    assert ba.ptr.value % 16 == (0 if aligned else 4)
    # the fused call; (d) two calls bit-equal; the second call of a (range pair, width) leaves plx_device_bytes alone
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == 0, nv.lib().plx_last_error()
    fam = family_of(lat)
    assert fam == expect(d, L), (label, fam)
    REACHED.update(fam)
    got_x, got_f = gx.cpu(bc, d).clone(), fl.cpu(bc, L).clone()
    bytes1 = lat.device_bytes
    gx2, fl2 = new_out(bc, d), new_out(bc, L)
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx2.ptr, fl2.ptr) == 0
    assert lat.device_bytes == bytes1, (label, "the second call of a range pair moved plx_device_bytes")
    assert torch.equal(gx2.cpu(bc, d), got_x) and torch.equal(fl2.cpu(bc, L), got_f), (label, "not deterministic")
    gx3 = new_out(bc, d)
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx3.ptr, None) == 0       # (e) d_filtered = NULL
    assert torch.equal(gx3.cpu(bc, d), got_x)
    # (a) the stack splat against splat_rows of the explicit half stack, one multiply per product element, all columns
    ta_, tx_ = ba.view.view(ac, L), bx.view.view(N, d)[ab:ab + ac]
    hs = torch.cat([ta_, (ta_[:, :, None] * tx_[:, None, :]).reshape(ac, L * d)], dim=1).contiguous()
    assert hs.shape == (ac, H) and hs.dtype == F32
    assert np.array_equal(hs.cpu().numpy(), half_stack64(a, x[ab:ab + ac]).astype(np.float32))
    values = Buf(count=lat.m * stride, dtype=F32, fill=SENTINEL)
    assert raw_splat(lat, ba.ptr, ab, ac, bx.ptr, L, values.ptr) == 0, nv.lib().plx_last_error()
    assert family_of(lat)[0] == fam[0]
    explicit = lat.splat_rows(hs, ab)
    assert explicit.shape == (lat.m, stride)
    assert torch.equal(values.view.view(lat.m, stride), explicit), (label, "stack splat differs from splat_rows(half stack)")
    # (b) filtered against columns [0, L) of apply_rows(half stack)
    assert torch.equal(got_f, lat.apply_rows(hs, ab, bb, bc)[:, :L].cpu()), (label, "filtered differs from apply_rows")
    # (c) staged against fused
    blurred = lat.blur(values.view.view(lat.m, stride), vd=H)
    gx4, fl4 = new_out(bc, d), new_out(bc, L)
    assert raw_contract(lat, ptr(blurred), bbuf.ptr, bb, bc, bx.ptr, L, gx4.ptr, fl4.ptr) == 0, nv.lib().plx_last_error()
    assert family_of(lat)[1] == fam[1]
    assert torch.equal(gx4.cpu(bc, d), got_x) and torch.equal(fl4.cpu(bc, L), got_f), (label, "staged differs from fused")
    # the other side: a and b swapped, for the comparison with the padded problem
    gx5 = new_out(ac, d)
    assert raw_apply(lat, bbuf.ptr, bb, bc, ba.ptr, ab, ac, bx.ptr, L, gx5.ptr, None) == 0, nv.lib().plx_last_error()
    assert family_of(lat) == fam
    other_x = gx5.cpu(ac, d).clone()
    # (f) nothing outside the outputs was written
    check_buffers(inputs=(ba, bbuf, bx), outputs=(gx, fl, gx2, fl2, gx3, gx4, fl4, gx5, values))
    # the two sides against the float64 square reference of the padded problem
    sides = scatter_sides(N, d, (bb, bc), (ab, ac), got_x.numpy(), other_x.numpy())
    bar_sq = 2 * (k + 4 * (L + 1)) * U32
    rp = ratio_to_bar(sides, sq_want, sq_T, bar_sq, label)
    rq = None
    if plx.Lattice.backward_fusable(L, d):
        A, B = cuda(padded(a, (ab, ac), N)), cuda(padded(b, (bb, bc), N))
        pad_x, _ = lat.apply_backward(A, B, bx.view.view(N, d).contiguous())
        rq = ratio_to_bar(pad_x.cpu().numpy(), sq_want, sq_T, bar_sq, label)
    # the bar: every entry of grad_x; filtered against the bar of the product
    bar_x, bar_f = (k + 2 * (L + 1)) * U32, k * U32
    rx = ratio_to_bar(got_x.numpy(), want, T, bar_x, label)
    rf = ratio_to_bar(got_f.numpy(), want_f.astype(LD), ta, bar_f, label)
    w = WORST.setdefault(fam, [0.0, 0.0, 0.0, 0])
    w[0], w[1], w[2], w[3] = max(w[0], rx), max(w[1], rf), max(w[2], rp), w[3] + 1
    print(f"{label}: k32 = {k}  grad_x / bar {rx:.4f} (bar {bar_x:.2e} T'')  filtered / bar {rf:.4f} (bar {bar_f:.2e} T)  "
          f"sides / square bar {rp:.4f}  fused padded call / square bar {'-' if rq is None else format(rq, '.4f')}  {fam}")
    assert rx <= 1.0, (label, "grad_x entry ratio to the bar", rx)
    assert rf <= 1.0, (label, "filtered entry ratio to the bar", rf)
    assert rp <= 1.0, (label, "the two sides against the float64 square reference, ratio to the bar", rp)
    assert rq is None or rq <= 1.0, (label, "Lattice.apply_backward on the padded matrices, ratio to the bar", rq)
    if kind == "isolated":
        zero = (T == 0).all(axis=1)
        assert zero.sum() >= bc // 2 and bool((got_x.numpy()[zero] == 0).all()), label


def test_column_limit_edge():
    """stride = 4096 exactly (d = 7, L = 512: 1024 chunks, 64 KiB of LDS per workgroup), the widest row the contraction
    holds.  grad_x is judged against the contraction in np.longdouble of the DEVICE's own filtered half stack, which the
    kernel's on-chip row equals bit for bit: what is left is the contraction alone, a recursive sum of 2 L products of at
    most three roundings each, so |got - want| <= (2 L + 4) 2^-24 T with T twice the sum of the absolute terms.  And one
    column past the limit (d = 1, L = 2049: stride 4100) is refused with nothing written."""
    d, L = 7, 512
    H = L * (1 + d)
    assert H == plx.Lattice.BACKWARD_ROWS_MAX_STRIDE and plx.Lattice.backward_rows_ok(L, d)
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    x = cloud("gauss1", N, d, seed=78, coeffs=dtaps).astype(np.float64)
    (ab, ac), (bb, bc) = ranges("head0.5", N)
    rng = np.random.default_rng(78)
    a, b = f32_values(rng, (ac, L)), f32_values(rng, (bc, L))
    lat = plx.Lattice().build(cuda(x), dtaps)
    ba, bbuf, bx = (Buf(t, offset=1, dtype=F32) for t in (a, b, x))
    gx, fl = Buf(count=bc * d, offset=1, dtype=F32, fill=SENTINEL), Buf(count=bc * L, offset=1, dtype=F32, fill=SENTINEL)
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == 0, nv.lib().plx_last_error()
    assert family_of(lat) == WIDE
    REACHED.update(WIDE)
    ta_, tx_ = ba.view.view(ac, L), bx.view.view(N, d)[ab:ab + ac]
    hs = torch.cat([ta_, (ta_[:, :, None] * tx_[:, None, :]).reshape(ac, L * d)], dim=1).contiguous()
    values = Buf(count=lat.m * H, dtype=F32, fill=SENTINEL)
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
    r = ratio_to_bar(gx.np(bc, d), want, T, (2 * L + 4) * 2.0 ** -24, "limit")
    print(f"column limit d={d} L={L}: grad_x against the contraction of the device's filtered half stack / bar {r:.4f}")
    assert r <= 1.0, r
    lat.close()
    # d = 1, L = 2049: H = 4098, stride 4100 (buffers of the full size: nothing could run past them)
    d1, Lw = 1, 2049
    assert not plx.Lattice.backward_rows_ok(Lw, d1) and plx.Lattice.backward_rows_ok(Lw - 1, d1)
    x1 = Buf(rng.standard_normal((N, d1)), dtype=F32)
    lat = plx.Lattice().build(x1.view.view(N, d1).contiguous(), dtaps)
    wide = Buf(count=N * Lw, dtype=F32, fill=0.5)
    gx1, fl_w = Buf(count=N * d1, dtype=F32, fill=SENTINEL), Buf(count=N * Lw, dtype=F32, fill=SENTINEL)
    values = Buf(count=lat.m * 4100, dtype=F32, fill=SENTINEL)
    bytes0 = lat.device_bytes
    err = nv.lib().plx_last_error
    full = (0, N)
    assert raw_splat(lat, wide.ptr, *full, x1.ptr, Lw, values.ptr) == PLX_ERR_INVALID and b"4096" in err()
    assert raw_contract(lat, values.ptr, wide.ptr, *full, x1.ptr, Lw, gx1.ptr, fl_w.ptr) == PLX_ERR_INVALID and b"4096" in err()
    assert raw_apply(lat, wide.ptr, *full, wide.ptr, *full, x1.ptr, Lw, gx1.ptr, fl_w.ptr) == PLX_ERR_INVALID and b"4096" in err()
    with pytest.raises(PlxError) as e:
        lat.apply_backward_rows_f32(wide.view.view(N, Lw), 0, wide.view.view(N, Lw), 0, x1.view.view(N, d1))
    assert e.value.code == PLX_ERR_INVALID and "4096" in str(e.value)
    assert lat.device_bytes == bytes0
    torch.cuda.synchronize()
    assert gx1.unchanged() and fl_w.unchanged() and values.unchanged()
    check_buffers(inputs=(wide, x1), outputs=(gx1, fl_w, values))
    lat.close()


def test_refusals_leave_the_outputs_untouched():
    d, L = 3, 2
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, d)).astype(np.float32)
    (ab, ac), (bb, bc) = ranges("head0.8", N)
    ba, bbuf = Buf(rng.standard_normal((ac, L)), dtype=F32), Buf(rng.standard_normal((bc, L)), dtype=F32)
    bx = Buf(x, dtype=F32)
    gx, fl = Buf(count=bc * d, dtype=F32, fill=SENTINEL), Buf(count=bc * L, dtype=F32, fill=SENTINEL)
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
    values = Buf(count=4096, dtype=F32, fill=SENTINEL)
    bytes0 = lat.device_bytes
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"not built" in err()
    assert lat.device_bytes == bytes0
    untouched(values)
    # one shard of two
    lat.build(cuda(x), dtaps, shard=(0, 2))
    bytes0 = lat.device_bytes
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"shard" in err()
    assert lat.device_bytes == bytes0
    untouched(values)
    lat.close()
    # a build that replayed the reference's table growth
    nv.check(nv.lib().plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        lat = plx.Lattice().build(cuda(x), dtaps)
    finally:
        nv.check(nv.lib().plx_tune(b"reference_growth", 0), "plx_tune")
    assert lat.reference_growth_info()["replayed"]
    bytes0 = lat.device_bytes
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"reference_growth" in err()
    assert lat.device_bytes == bytes0
    with pytest.raises(PlxError) as e:
        lat.apply_backward_rows_f32(ba.view.view(ac, L), ab, bbuf.view.view(bc, L), bb, bx.view.view(N, d))
    assert e.value.code == PLX_ERR_STATE
    untouched(values)
    lat.close()
    # on a plain build: d_values off 16-byte alignment
    lat = plx.Lattice().build(cuda(x), dtaps)
    bytes0 = lat.device_bytes
    stride = stride_of(d, L)
    values = Buf(count=lat.m * stride, offset=1, dtype=F32, fill=SENTINEL)
    assert values.ptr.value % 16 == 4
    assert raw_splat(lat, ba.ptr, ab, ac, bx.ptr, L, values.ptr) == PLX_ERR_INVALID and b"16-byte" in err()
    assert raw_contract(lat, values.ptr, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"16-byte" in err()
    untouched(values)
    # a range past n, a negative begin, a count < 1 -- on either side
    values = Buf(count=lat.m * stride, dtype=F32, fill=SENTINEL)
    for bad in ((N - 3, 4), (-1, 4), (0, N + 1), (0, 0)):
        # only the calls that take the bad range: the third would be a valid call, and run
        assert raw_splat(lat, ba.ptr, bad[0], bad[1], bx.ptr, L, values.ptr) == PLX_ERR_INVALID, bad
        assert raw_apply(lat, ba.ptr, bad[0], bad[1], bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID, bad
        assert raw_contract(lat, values.ptr, bbuf.ptr, bad[0], bad[1], bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID, bad
        assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bad[0], bad[1], bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID, bad
    assert raw_splat(lat, ba.ptr, N - 3, 4, bx.ptr, L, values.ptr) == PLX_ERR_INVALID and b"range" in err()
    with pytest.raises(ValueError, match="range"):
        lat.apply_backward_rows_f32(ba.view.view(ac, L), N - 3, bbuf.view.view(bc, L), bb, bx.view.view(N, d))
    # the lattice-free refusals once more, next to a real lattice
    assert all_three(lat, values, nrhs=0) == (PLX_ERR_INVALID,) * 3 and b"positive" in err()
    assert raw_apply(lat, None, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, None, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, None, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, None, fl.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_splat(lat, ba.ptr, ab, ac, bx.ptr, L, None) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_contract(lat, None, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, ctypes.c_void_p(bx.ptr.value + 2), L, gx.ptr,
                     fl.ptr) == PLX_ERR_INVALID and b"4-byte" in err()
    assert raw_apply(lat, gx.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, fl.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_apply(lat, ba.ptr, ab, ac, bbuf.ptr, bb, bc, bx.ptr, L, gx.ptr, gx.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_contract(lat, values.ptr, bbuf.ptr, bb, bc, bx.ptr, L, values.ptr, None) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_splat(lat, ba.ptr, ab, ac, values.ptr, L, values.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert lat.device_bytes == bytes0
    untouched(values)
    lat.close()


def test_too_large_is_refused_before_any_work():
    """a_count * stride = 2^31 exactly: n = 2^19 points on a line (d = 1), 2048 columns, stride 4096.  a and b are one
    uninitialised allocation of the full n x 2048 size, so that nothing could be read past its end; no output may be
    written."""
    n, d, L = 1 << 19, 1, 2048
    assert plx.Lattice.backward_rows_ok(L, d)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(1)).cuda()
    lat = plx.Lattice().build(x, dkernel("rbf", 1).get_deriv_coeffs().numpy())
    big = torch.empty((n, L), dtype=F32, device="cuda")
    gx = Buf(count=n * d, dtype=F32, fill=SENTINEL)
    values = Buf(count=64, dtype=F32, fill=SENTINEL)
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
    lat = plx.Lattice().build(x, dtaps)
    gx, fl = torch.full((bc, d), SENTINEL, dtype=F32, device="cuda"), torch.full((bc, L), SENTINEL, dtype=F32, device="cuda")
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
        eager_x, eager_f = lat.apply_backward_rows_f32(a, ab, b, bb, x)       # the warm-up: tables and workspace
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
        assert lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


# ---- operator level -------------------------------------------------------------------------------------------------
N_IN, N_OUT = 140, 561
LS = 0.75


@pytest.fixture
def native_rows_grad_on():
    before = plx.RectangularLazyLattice.native_rows_grad
    plx.RectangularLazyLattice.native_rows_grad = True
    yield
    plx.RectangularLazyLattice.native_rows_grad = before
    plx.lattice_cache().clear()


def _cached_rows_kernels():
    names = set()
    for lat, _, _ in plx.lattice_cache()._entries.values():
        fam = lat.rows_kernels()
        names.update(fam["splat"] + fam["slice"])
    return names


def _operator_grads(dk, xin, xout, v, w, native, transposed):
    """(stacked positions as the device formed them, x_in.grad, x_out.grad, ls.grad, V.grad, rows kernels seen on the cached
    lattices) of (K V . W).sum().backward() for K = RectangularLazyLattice(x_in / ls, x_out / ls) or, transposed, its
    _transpose_nonbatch() (V then lives on x_in)."""
    plx.RectangularLazyLattice.native_rows_grad = native
    plx.lattice_cache().clear()
    ti, to, tv = (cuda(t).requires_grad_(True) for t in (xin, xout, v))
    ls = torch.tensor([LS], dtype=F32, device="cuda", requires_grad=True)
    op = plx.RectangularLazyLattice(ti / ls, to / ls, dk)
    stacked = torch.cat((op.xout, op.xin)).detach().cpu().numpy()
    if transposed:
        op = op._transpose_nonbatch()
    out = op._matmul(tv)
    (out * cuda(w)).sum().backward()
    names = _cached_rows_kernels()
    return stacked, ti.grad.cpu().numpy(), to.grad.cpu().numpy(), float(ls.grad), tv.grad.cpu().numpy(), names


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("profile", ["rbf", "matern32"])
@pytest.mark.parametrize("d,L", [(3, 2), (8, 1)])
def test_autograd_native_against_padded(native_rows_grad_on, d, L, profile, transposed):
    """The gradients of (K(x_in / ls, x_out / ls) V . W).sum() with respect to the fp32 leaves x_in, x_out, ls and V, with
    native_rows_grad on and off.  With p = [x_out; x_in] / ls the stacked positions, T' the size of the terms of p.grad
    (tests/test_backward_f64_gpu.reference on the padded problem) and B = (k32 + 4 (L + 1)) 2^-23 T' the bar of one route
    (each one-sided call: (k32 + 2 (L + 1)) 2^-23 T''; the padded route filters the same stack at the same depth), the two
    routes' p.grad differ by at most 2 B.  x.grad = p.grad / ls adds at most two roundings per route, each 2^-24 of a value
    no larger than T' / ls:   |x.grad native - x.grad padded| <= (2 B + 2 * 2^-23 T') / ls.
    ls.grad = -sum_ik p.grad[i][k] x[i][k] / ls^2 is a sum of n d terms of at most T' |p| / ls each (|p| = |x| / ls): the
    routes' terms differ by 2 B |p| / ls plus three roundings each (a product, a square, a division), and each route's sums
    (one per leaf, then added), in whatever order, add at most n d + 1 roundings of the sum of the absolute terms:
        |ls.grad native - ls.grad padded| <= (2 (k32 + 4 (L + 1)) + 2 (n d + 4)) 2^-23 sum_ik T' |p| / ls.
    V.grad: rel-L2 between the routes within REL, the bar of the fp32 forward product (tests/test_backward_fp64.py).  The
    native run reports the new kernels, the padded run none of them."""
    dk = dkernel(profile, 1)
    dtaps = dk.get_deriv_coeffs().numpy()
    x = cloud("gauss1", N, d, seed=3 * d + L, coeffs=dtaps) * np.float32(LS)          # p = x / ls is the cloud, to rounding
    xout, xin = x[:N_OUT], x[N_OUT:]
    rng = np.random.default_rng(10 * d + L)
    src_rng, out_rng = ((N_OUT, N_IN), (0, N_OUT)) if transposed else ((0, N_OUT), (N_OUT, N_IN))
    v, w = f32_values(rng, (src_rng[1], L)), f32_values(rng, (out_rng[1], L))
    res = {native: _operator_grads(dk, xin, xout, v, w, native, transposed) for native in (True, False)}
    assert set(expect(d, L)) <= res[True][5], res[True][5]                   # the native route ran the new kernels ...
    assert not set(CHUNK + WIDE) & res[False][5], res[False][5]              # ... and the padded route did not
    REACHED.update(res[True][5] & set(CHUNK + WIDE))
    p = res[True][0].astype(np.float64)
    assert np.array_equal(res[True][0], res[False][0])
    l64 = Lattice64(p, dtaps)
    _, _, T, _ = reference(padded(w, out_rng, N), padded(v, src_rng, N), p, l64)
    k = k32(l64)
    route = (k + 4 * (L + 1)) * U32
    bar_x = (2 * route + 2 * U32) * T / LS
    gx = {native: np.concatenate([r[2], r[1]]) for native, r in res.items()}     # rows of the stacked points
    err_x = np.abs(gx[True].astype(np.float64) - gx[False].astype(np.float64))
    rx = float(np.max(np.where(bar_x > 0, err_x / np.where(bar_x > 0, bar_x, 1.0), np.where(err_x > 0, np.inf, 0.0))))
    bar_ls = (2 * (k + 4 * (L + 1)) + 2 * (N * d + 4)) * U32 * float((T * np.abs(p)).sum()) / LS
    rl = abs(res[True][3] - res[False][3]) / bar_ls
    rv = rel_l2(res[True][4], res[False][4].astype(np.float64))
    print(f"autograd fp32 d={d} L={L} {profile} transposed={transposed}: native against padded, x.grad / bar {rx:.4f}  "
          f"ls.grad / bar {rl:.4f}  V.grad rel-L2 {rv:.2e} (bar {REL:.1e})")
    assert np.all(np.isfinite(gx[True])) and np.isfinite(res[True][3])
    assert rx <= 1.0, ("x_in.grad / x_out.grad", rx)
    assert rl <= 1.0, ("ls.grad", rl)
    assert rv <= REL, ("V.grad", rv)


def test_switch_off_reports_none_of_the_new_kernels():
    """The default: an fp32 product whose positions want a gradient takes the padded route."""
    assert plx.RectangularLazyLattice.native_rows_grad is False
    d, L = 3, 2
    dk = dkernel("rbf", 1)
    x = cloud("gauss1", N, d, seed=5, coeffs=dk.get_deriv_coeffs().numpy())
    rng = np.random.default_rng(1)
    res = _operator_grads(dk, x[N_OUT:], x[:N_OUT], f32_values(rng, (N_OUT, L)), f32_values(rng, (N_IN, L)), False, False)
    assert not set(CHUNK + WIDE) & res[5], res[5]
    plx.lattice_cache().clear()


def family_report():
    lines = ["one-sided fp32 position gradient against Lattice64, worst ratio to the bar per kernel family "
             "(grad_x, filtered, two sides against the float64 square reference):"]
    for fam, (a, b, c, cases) in sorted(WORST.items()):
        lines.append(f"  {fam[0]} | {fam[1]}: {a:.4f} {b:.4f} {c:.4f} ({cases} cases)")
    return "\n".join(lines)


def test_every_new_kernel_was_launched():
    """Every kernel name plx_rows_backward.hip can report ran in this module (run as a whole)."""
    print(family_report())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "simplex_gp_amd", "csrc", "plx_rows_backward.hip")).read()
    literals = set()
    for stmt in re.finditer(r"\bk(?:Splat|Contract)(?:Chunk|Wide)\s*=([^;]*);", text):
        literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    assert literals == set(CHUNK + WIDE), literals
    assert REACHED == literals, sorted(literals - REACHED)
    for lat in (v[-1] for v in _REF.values()):
        lat.close()
    _REF.clear()
