"""The float64 position gradient (plx_backward_splat_f64 / plx_backward_contract_f64 / plx_apply_backward_f64,
simplex_gp_amd/csrc/plx_backward_f64.hip) on the GPU.

Yardstick: tests/lattice64 -- the stacked matrix stack64(g, src, x) in float64, filtered by Lattice64 on the derivative-tap
lattice of x rounded to float32, the contraction redone in np.longdouble.  x is a float64 matrix that is NOT representable
in float32 (a relative 1e-9 is added), so a stack formed from the rounded copy shows.

Contract (i), bits (torch.equal): the stack splat against Lattice.splat of the explicit stacked matrix (formed on the device
in double, one multiply per product element); grad_src against columns [0, L) of Lattice.apply of it; staged against fused;
two calls; plx_device_bytes on the second call of a width.

Contract (ii), the bar, derived, per entry of grad_x, with k = depth(lat) as in tests/test_f64_gpu.py:
    |got - want| <= 2 (k + 4 (L + 1)) 2^-52 T'[p, k]
    T' = 2 sum_l ( |s_l x_k| t(g)_l + |s_l| t(g (x) x)_lk + |g_l x_k| t(s)_l + |g_l| t(s (x) x)_lk ),   t(.) = Lattice64.terms64
Every filtered entry carries at most k roundings of its own terms (the stack product is one of them), the contraction adds at
most two multiplies and 4 L additions, the factor 2 covers the float64 filter of the reference, which obeys the same bound.
Where T' = 0 the result must be exactly 0; no entry is left out.  grad_src per entry: k 2^-52 terms64(g) (DESIGN.md section
14).  Worst ratios per kernel family are printed at the end (pytest -s) and copied to profiles/backward_f64_measured.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import solvers
from simplex_gp_amd._native import PlxError
from simplex_gp_amd.stencil import Matern, rbf
from tests.gpubuf import SENTINEL, Buf, check_buffers
from tests.lattice64 import Lattice64, cloud, stack64

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -52
N = 701
PLX_ERR_INVALID, PLX_ERR_STATE, PLX_ERR_TOO_LARGE = 1, 5, 6
F64 = torch.float64
LD = np.longdouble
CHUNK = ("f64_backward_splat_chunk_kernel", "f64_backward_contract_chunk_kernel")
WIDE = ("f64_backward_splat_wide_kernel", "f64_backward_contract_wide_kernel")

# (d, L, derivative-tap order, profile, cloud, buffers 16-byte aligned): every kernel form and the 64 / 65-chunk switch
CASES = [
    (1, 1, 0, "rbf", "gauss1", True),            # 2 chunks, the smallest row
    (3, 2, 1, "rbf", "simplex", False),          # vertex rows of n corners
    (8, 3, 2, "matern32", "dup", True),
    (3, 16, 3, "matern32", "gauss1", False),     # 64 chunks: the last chunk shape
    (4, 13, 1, "rbf", "isolated", True),         # 65 chunks: the first wide shape; the true gradient vanishes
    (8, 11, 1, "rbf", "gauss1", False),          # 99 chunks, the training shape
    (18, 1, 1, "matern32", "gauss1", True),
    (18, 4, 0, "rbf", "gauss1", False),
    (24, 1, 2, "rbf", "gauss1", False),          # d + 1 > 20: the run-time form, chunk
    (24, 3, 1, "matern32", "gauss1", True),      # ... and wide
]
IDS = [f"d{d}-L{L}-o{o}-{p}-{c}-{'al' if a else 'off'}" for d, L, o, p, c, a in CASES]

_DK, _REF = {}, {}
WORST = {}            # family -> [grad_x ratio to its bar, grad_src ratio to its bar, cases]
REACHED = set()


def expect(d, L):
    return CHUNK if L * (1 + d) <= 64 else WIDE


def dkernel(profile, order):
    if (profile, order) not in _DK:
        fn = rbf if profile == "rbf" else (lambda d2: Matern.apply(d2, 1.5))
        _DK[(profile, order)] = plx.DiscretizedKernelFN(fn, order)
    return _DK[(profile, order)]


def cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def depth(lat):
    """k of tests/test_f64_gpu.py: the additions and multiplications along the deepest path of the fp64 product."""
    row_ptr = lat.export(nv.ARRAY_ROW_PTR).astype(np.int64)
    lmax = int(np.diff(row_ptr).max())
    d, r = lat.d, lat.order
    return lmax + (2 * r + 1) * (d + 1) + 2 * (d + 1) + 8


def positions64(kind, n, d, seed, coeffs):
    """float64 positions whose rounding to float32 is the named cloud, and which differ from it in the low bits."""
    x32 = cloud(kind, n, d, seed=seed, coeffs=coeffs)
    rng = np.random.default_rng(seed + 100)
    x = x32.astype(np.float64) * (1.0 + 1e-9 * rng.standard_normal(x32.shape))
    assert np.array_equal(x.astype(np.float32), x32) and not np.array_equal(x, x32.astype(np.float64))
    return x


def reference(g, src, x, l64):
    """(grad_x in longdouble from the float64-filtered stack, grad_src, T', terms64(g)): computed once per case."""
    n, L = g.shape
    d = x.shape[1]
    stack = stack64(g, src, x)
    f = l64.apply_staged(stack)
    t = l64.terms64(stack)
    wg, wgx, ws, wsx = (a.astype(LD) for a in np.split(f, [L, L + L * d, 2 * L + L * d], axis=1))
    tg, tgx, ts, tsx = np.split(t, [L, L + L * d, 2 * L + L * d], axis=1)
    wgx, wsx, tgx, tsx = (a.reshape(n, L, d) for a in (wgx, wsx, tgx, tsx))
    s3, g3, x3 = src.astype(LD)[:, :, None], g.astype(LD)[:, :, None], x.astype(LD)[:, None, :]
    want = -2 * (s3 * x3 * wg[:, :, None] - s3 * wgx + g3 * x3 * ws[:, :, None] - g3 * wsx).sum(1)
    a3, b3, y3 = np.abs(src)[:, :, None], np.abs(g)[:, :, None], np.abs(x)[:, None, :]
    T = 2.0 * (a3 * y3 * tg[:, :, None] + a3 * tgx + b3 * y3 * ts[:, :, None] + b3 * tsx).sum(1)
    return want, f[:, :L].copy(), T, tg.copy()


def ratio_to_bar(got, want, T, bar, label):
    """max |got - want| / (bar T) over EVERY entry; where T = 0 the entry must be exactly 0 (else inf)."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape == T.shape and np.all(np.isfinite(got)), label
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    zero = T == 0
    if np.any(got[zero] != 0):
        return float("inf")
    return float((err[~zero] / (bar * T[~zero])).max()) if np.any(~zero) else 0.0


def case_data(idx):
    """Everything a case needs, built once for the module: inputs, the yardstick, the GPU lattice."""
    if idx not in _REF:
        d, L, order, profile, kind, aligned = CASES[idx]
        dtaps = dkernel(profile, order).get_deriv_coeffs().numpy()
        x = positions64(kind, N, d, seed=idx + 1, coeffs=dtaps)
        rng = np.random.default_rng(1000 + idx)
        g, src = rng.standard_normal((N, L)), rng.standard_normal((N, L))
        if kind == "isolated":
            g[::2] = 0.0                               # rows no term reaches: T' = 0 there, and so must the gradient be
            src[::2] = 0.0
        l64 = Lattice64(x, dtaps)
        lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
        assert lat.m == l64.m and lat.order == order
        _REF[idx] = (g, src, x, reference(g, src, x, l64), lat)
    return _REF[idx]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_splat(lat, g, s, x, L, values, stream=None):
    return nv.lib().plx_backward_splat_f64(lat._h, g, s, x, L, values, stream or stream_ptr())


def raw_contract(lat, values, g, s, x, L, gx, gs, stream=None):
    return nv.lib().plx_backward_contract_f64(lat._h, values, g, s, x, L, gx, gs, stream or stream_ptr())


def raw_apply(lat, g, s, x, L, gx, gs, stream=None):
    return nv.lib().plx_apply_backward_f64(lat._h, g, s, x, L, gx, gs, stream or stream_ptr())


def family_of(lat):
    k = lat.f64_kernels()
    return ("+".join(k["splat"]), "+".join(k["slice"]))


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_backward_f64_against_lattice64(idx):
    d, L, order, profile, kind, aligned = CASES[idx]
    g, src, x, (want, want_gs, T, tg), lat = case_data(idx)
    C, off, label = 2 * L * (1 + d), 0 if aligned else 1, IDS[idx]
    bg, bs, bx = (Buf(a, offset=off, dtype=F64) for a in (g, src, x))
    gx, gs = Buf(count=N * d, offset=off, dtype=F64, fill=SENTINEL), Buf(count=N * L, offset=off, dtype=F64, fill=SENTINEL)
    assert bg.ptr.value % 16 == (0 if aligned else 8)
    # the fused call; two calls bit-equal; the second call of a width leaves plx_device_bytes alone
    assert raw_apply(lat, bg.ptr, bs.ptr, bx.ptr, L, gx.ptr, gs.ptr) == 0, nv.lib().plx_last_error()
    fam = family_of(lat)
    assert fam == expect(d, L), (label, fam)
    assert lat.f64_kernels()["blur_axis"] == ["f64_blur_chunk_kernel"]
    REACHED.update(fam)
    got_x, got_s = gx.cpu(N, d).clone(), gs.cpu(N, L).clone()
    bytes1 = lat.device_bytes
    gx2, gs2 = Buf(count=N * d, offset=off, dtype=F64, fill=SENTINEL), Buf(count=N * L, offset=off, dtype=F64, fill=SENTINEL)
    assert raw_apply(lat, bg.ptr, bs.ptr, bx.ptr, L, gx2.ptr, gs2.ptr) == 0
    assert lat.device_bytes == bytes1, (label, "the second call of a width moved plx_device_bytes")
    assert torch.equal(gx2.cpu(N, d), got_x) and torch.equal(gs2.cpu(N, L), got_s), (label, "not deterministic")
    # d_grad_src = NULL: the same grad_x, nothing else written
    gx3 = Buf(count=N * d, offset=off, dtype=F64, fill=SENTINEL)
    assert raw_apply(lat, bg.ptr, bs.ptr, bx.ptr, L, gx3.ptr, None) == 0
    assert torch.equal(gx3.cpu(N, d), got_x)
    # contract (i): the stack splat against Lattice.splat of the explicit stack, one multiply per product element
    tg_, ts_, tx_ = bg.view.view(N, L), bs.view.view(N, L), bx.view.view(N, d)
    stack = torch.cat([tg_, (tg_[:, :, None] * tx_[:, None, :]).reshape(N, L * d),
                       ts_, (ts_[:, :, None] * tx_[:, None, :]).reshape(N, L * d)], dim=1).contiguous()
    assert stack.shape == (N, C) and np.array_equal(stack.cpu().numpy(), stack64(g, src, x))
    values = Buf(count=lat.m * C, dtype=F64, fill=SENTINEL)
    assert raw_splat(lat, bg.ptr, bs.ptr, bx.ptr, L, values.ptr) == 0, nv.lib().plx_last_error()
    assert torch.equal(values.view.view(lat.m, C), lat.splat(stack)), (label, "stack splat differs from splat(stack)")
    # ... grad_src against columns [0, L) of apply(stack)
    assert torch.equal(got_s, lat.apply(stack)[:, :L].cpu()), (label, "grad_src differs from apply(stack)[:, :L]")
    # ... staged against fused
    assert raw_splat(lat, bg.ptr, bs.ptr, bx.ptr, L, values.ptr) == 0
    blurred = lat.blur(values.view.view(lat.m, C), vd=C)
    gx4, gs4 = Buf(count=N * d, offset=off, dtype=F64, fill=SENTINEL), Buf(count=N * L, offset=off, dtype=F64, fill=SENTINEL)
    assert raw_contract(lat, ptr(blurred), bg.ptr, bs.ptr, bx.ptr, L, gx4.ptr, gs4.ptr) == 0, nv.lib().plx_last_error()
    assert family_of(lat) == fam
    assert torch.equal(gx4.cpu(N, d), got_x) and torch.equal(gs4.cpu(N, L), got_s), (label, "staged differs from fused")
    check_buffers(inputs=(bg, bs, bx), outputs=(gx, gs, gx2, gs2, gx3, gx4, gs4, values))
    # contract (ii): every entry of grad_x against the bar; grad_src against the bar of the product
    k = depth(lat)
    bar_x, bar_s = 2 * (k + 4 * (L + 1)) * U2, k * U2
    rx = ratio_to_bar(got_x.numpy(), want, T, bar_x, label)
    rs = ratio_to_bar(got_s.numpy(), want_gs.astype(LD), tg, bar_s, label)
    w = WORST.setdefault(fam, [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], rx), max(w[1], rs), w[2] + 1
    print(f"{label}: k = {k}  grad_x / bar {rx:.3f} (bar {bar_x:.2e} T')  grad_src / bar {rs:.3f} (bar {bar_s:.2e} T)  {fam}")
    assert rx <= 1.0, (label, "grad_x entry ratio to the bar", rx)
    assert rs <= 1.0, (label, "grad_src entry ratio to the bar", rs)
    if kind == "isolated":
        zero = (T == 0).all(axis=1)
        assert zero.sum() >= N // 2 and bool((got_x.numpy()[zero] == 0).all()), label
        assert float(np.abs(got_x.numpy()).max()) <= bar_x * float(T.max()), (label, "the true gradient vanishes")


def test_column_limit_edge():
    """C = 2048 exactly (d = 7, L = 128: 1024 chunks, 64 KiB of LDS per workgroup), the widest row the contraction holds.
    The bit contracts as everywhere.  grad_x is judged against the contraction in np.longdouble of the DEVICE's own filtered
    stack, which the kernel's on-chip row equals bit for bit: what is left is the contraction alone, a sum of 4 L products
    of at most two roundings each taken in sequence, so |got - want| <= (4 L + 4) 2^-53 T with T twice the sum of the
    absolute terms (the standard bound of a recursive sum, first order)."""
    d, L = 7, 128
    C = 2 * L * (1 + d)
    assert C == plx.Lattice.BACKWARD_F64_MAX_COLUMNS
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    x = positions64("gauss1", N, d, seed=77, coeffs=dtaps)
    rng = np.random.default_rng(77)
    g, src = rng.standard_normal((N, L)), rng.standard_normal((N, L))
    lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
    bg, bs, bx = (Buf(a, offset=1, dtype=F64) for a in (g, src, x))
    gx, gs = Buf(count=N * d, offset=1, dtype=F64, fill=SENTINEL), Buf(count=N * L, offset=1, dtype=F64, fill=SENTINEL)
    assert raw_apply(lat, bg.ptr, bs.ptr, bx.ptr, L, gx.ptr, gs.ptr) == 0, nv.lib().plx_last_error()
    assert family_of(lat) == WIDE
    stack = cuda(stack64(g, src, x))
    values = Buf(count=lat.m * C, dtype=F64, fill=SENTINEL)
    assert raw_splat(lat, bg.ptr, bs.ptr, bx.ptr, L, values.ptr) == 0
    assert torch.equal(values.view.view(lat.m, C), lat.splat(stack))
    f = lat.apply(stack).cpu().numpy()
    assert np.array_equal(gs.np(N, L), f[:, :L])
    check_buffers(inputs=(bg, bs, bx), outputs=(gx, gs, values))
    wg, wgx, ws, wsx = (a.astype(LD) for a in np.split(f, [L, L + L * d, 2 * L + L * d], axis=1))
    wgx, wsx = wgx.reshape(N, L, d), wsx.reshape(N, L, d)
    s3, g3, x3 = src.astype(LD)[:, :, None], g.astype(LD)[:, :, None], x.astype(LD)[:, None, :]
    t1, t2, t3, t4 = s3 * x3 * wg[:, :, None], s3 * wgx, g3 * x3 * ws[:, :, None], g3 * wsx
    want = -2 * (t1 - t2 + t3 - t4).sum(1)
    T = (2 * (np.abs(t1) + np.abs(t2) + np.abs(t3) + np.abs(t4)).sum(1)).astype(np.float64)
    r = ratio_to_bar(gx.np(N, d), want, T, (4 * L + 4) * 2.0 ** -53, "limit")
    print(f"column limit d={d} L={L}: grad_x against the contraction of the device's filtered stack / bar {r:.3f}")
    assert r <= 1.0, r
    lat.close()


def test_refusals_leave_the_outputs_untouched():
    d, L = 3, 2
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, d))
    bg, bs = (Buf(rng.standard_normal((N, L)), dtype=F64) for _ in range(2))
    bx = Buf(x, dtype=F64)
    gx, gs = Buf(count=N * d, dtype=F64, fill=SENTINEL), Buf(count=N * L, dtype=F64, fill=SENTINEL)
    err = nv.lib().plx_last_error

    def all_three(lat, values, nrhs=L, g=bg, s=bs):
        return (raw_splat(lat, g.ptr, s.ptr, bx.ptr, nrhs, values.ptr),
                raw_contract(lat, values.ptr, g.ptr, s.ptr, bx.ptr, nrhs, gx.ptr, gs.ptr),
                raw_apply(lat, g.ptr, s.ptr, bx.ptr, nrhs, gx.ptr, gs.ptr))

    def untouched(*more):
        torch.cuda.synchronize()
        assert all(b.unchanged() for b in (gx, gs) + more), "a refused call wrote an output"
        check_buffers(inputs=(bg, bs, bx), outputs=(gx, gs) + more)

    # a lattice that is not built
    lat = plx.Lattice()
    values = Buf(count=4096, dtype=F64, fill=SENTINEL)
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"not built" in err()
    untouched(values)
    # one shard of two
    lat.build(cuda(x, np.float32), dtaps, shard=(0, 2))
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"shard" in err()
    with pytest.raises(PlxError) as e:
        lat.apply_backward(bg.view.view(N, L)[:lat.n_owned], bs.view.view(N, L)[:lat.n_owned], bx.view.view(N, d)[:lat.n_owned])
    assert e.value.code == PLX_ERR_STATE
    untouched(values)
    lat.close()
    # a build that replayed the reference's table growth
    nv.check(nv.lib().plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
    finally:
        nv.check(nv.lib().plx_tune(b"reference_growth", 0), "plx_tune")
    assert lat.reference_growth_info()["replayed"]
    assert all_three(lat, values) == (PLX_ERR_STATE,) * 3 and b"reference_growth" in err()
    untouched(values)
    lat.close()
    # on a plain build: d_values off 16-byte alignment; the lattice-free refusals once more, next to a real lattice
    lat = plx.Lattice().build(cuda(x, np.float32), dtaps)
    C = 2 * L * (1 + d)
    values = Buf(count=lat.m * C, offset=1, dtype=F64, fill=SENTINEL)
    assert values.ptr.value % 16 == 8
    assert raw_splat(lat, bg.ptr, bs.ptr, bx.ptr, L, values.ptr) == PLX_ERR_INVALID and b"16-byte" in err()
    assert raw_contract(lat, values.ptr, bg.ptr, bs.ptr, bx.ptr, L, gx.ptr, gs.ptr) == PLX_ERR_INVALID and b"16-byte" in err()
    values = Buf(count=lat.m * C, dtype=F64, fill=SENTINEL)
    assert all_three(lat, values, nrhs=0) == (PLX_ERR_INVALID,) * 3 and b"positive" in err()
    assert raw_apply(lat, None, bs.ptr, bx.ptr, L, gx.ptr, gs.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, bg.ptr, bs.ptr, bx.ptr, L, None, gs.ptr) == PLX_ERR_INVALID and b"NULL" in err()
    assert raw_apply(lat, bg.ptr, bs.ptr, ctypes.c_void_p(bx.ptr.value + 4), L, gx.ptr, gs.ptr) == PLX_ERR_INVALID
    assert b"8-byte" in err()
    assert raw_apply(lat, gx.ptr, bs.ptr, bx.ptr, L, gx.ptr, gs.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_apply(lat, bg.ptr, bs.ptr, bx.ptr, L, gx.ptr, gx.ptr) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_contract(lat, values.ptr, bg.ptr, bs.ptr, bx.ptr, L, values.ptr, None) == PLX_ERR_INVALID and b"alias" in err()
    assert raw_splat(lat, bg.ptr, bs.ptr, values.ptr, L, values.ptr) == PLX_ERR_INVALID and b"alias" in err()
    untouched(values)
    # the column limit: 2 * 257 * 4 = 2056 > 2048 (buffers of the full size: nothing could run past them)
    assert not plx.Lattice.backward_f64_ok(257, d) and plx.Lattice.backward_f64_ok(256, d)
    wide = Buf(count=N * 257, dtype=F64, fill=0.5)
    gs_w = Buf(count=N * 257, dtype=F64, fill=SENTINEL)
    values = Buf(count=lat.m * 2056, dtype=F64, fill=SENTINEL)
    bytes0 = lat.device_bytes
    assert raw_splat(lat, wide.ptr, wide.ptr, bx.ptr, 257, values.ptr) == PLX_ERR_INVALID and b"2048" in err()
    assert raw_contract(lat, values.ptr, wide.ptr, wide.ptr, bx.ptr, 257, gx.ptr, gs_w.ptr) == PLX_ERR_INVALID and b"2048" in err()
    assert raw_apply(lat, wide.ptr, wide.ptr, bx.ptr, 257, gx.ptr, gs_w.ptr) == PLX_ERR_INVALID and b"2048" in err()
    with pytest.raises(PlxError) as e:
        lat.apply_backward(wide.view.view(N, 257), wide.view.view(N, 257), bx.view.view(N, d))
    assert e.value.code == PLX_ERR_INVALID
    assert lat.device_bytes == bytes0
    untouched(values, gs_w)
    lat.close()


def test_too_large_is_refused_before_any_work():
    """n * C = 2^31 exactly: n = 2^20 points on a line (d = 1), 512 columns, C = 2048.  The inputs are one uninitialised
    allocation of the full n x 512 size, so that nothing could be read past its end; no output may be written."""
    n, d, L = 1 << 20, 1, 512
    assert plx.Lattice.backward_f64_ok(L, d)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(1), dtype=F64).cuda()
    lat = plx.Lattice().build(x.float(), dkernel("rbf", 1).get_deriv_coeffs().numpy())
    big = torch.empty((n, L), dtype=F64, device="cuda")
    gx = Buf(count=n * d, dtype=F64, fill=SENTINEL)
    values = Buf(count=64, dtype=F64, fill=SENTINEL)
    bytes0 = lat.device_bytes
    assert raw_apply(lat, ptr(big), ptr(big), ptr(x), L, gx.ptr, None) == PLX_ERR_TOO_LARGE
    assert b"2^31" in nv.lib().plx_last_error()
    assert raw_splat(lat, ptr(big), ptr(big), ptr(x), L, values.ptr) == PLX_ERR_TOO_LARGE
    assert raw_contract(lat, values.ptr, ptr(big), ptr(big), ptr(x), L, gx.ptr, None) == PLX_ERR_TOO_LARGE
    torch.cuda.synchronize()
    assert lat.device_bytes == bytes0 and gx.unchanged() and values.unchanged()
    check_buffers(outputs=(gx, values))
    lat.close()


def test_capture():
    d, L = 4, 3
    n = 5000
    dtaps = dkernel("rbf", 1).get_deriv_coeffs().numpy()
    rng = np.random.default_rng(9)
    x = cuda(rng.standard_normal((n, d)))
    g, s = cuda(rng.standard_normal((n, L))), cuda(rng.standard_normal((n, L)))
    lat = plx.Lattice().build(x.float(), dtaps)
    gx, gs = torch.full((n, d), SENTINEL, dtype=F64, device="cuda"), torch.full((n, L), SENTINEL, dtype=F64, device="cuda")
    bytes0 = lat.device_bytes
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    # the first call of a width under capture is refused, and nothing is written
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        rc = raw_apply(lat, ptr(g), ptr(s), ptr(x), L, ptr(gx), ptr(gs))
    assert rc == PLX_ERR_STATE and b"captured" in nv.lib().plx_last_error()
    del graph
    torch.cuda.synchronize()
    assert lat.device_bytes == bytes0
    assert bool((gx == SENTINEL).all()) and bool((gs == SENTINEL).all())
    with torch.cuda.stream(st):
        eager_x, eager_s = lat.apply_backward(g, s, x)              # the warm-up: tables and workspace
        first = lat.device_bytes
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            rc = raw_apply(lat, ptr(g), ptr(s), ptr(x), L, ptr(gx), ptr(gs))
        assert rc == 0, nv.lib().plx_last_error()
        graph.replay()
        st.synchronize()
        assert torch.equal(gx, eager_x) and torch.equal(gs, eager_s)
        # ... also on new inputs
        g2 = cuda(rng.standard_normal((n, L)))
        want_x, want_s = lat.apply_backward(g2, s, x)
        g.copy_(g2)
        graph.replay()
        st.synchronize()
        assert torch.equal(gx, want_x) and torch.equal(gs, want_s)
        assert lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


def _autograd(dk, x, v, w, fused):
    plx.LatticeFilterGeneral.fused_backward_f64 = fused
    xt, vt = cuda(x).requires_grad_(True), cuda(v).requires_grad_(True)
    out = plx.LatticeFilterGeneral.apply(vt, xt, dk)
    (out * cuda(w)).sum().backward()
    lat = plx.lattice_cache().get(xt.detach(), dk.get_deriv_coeffs().numpy())     # the lattice the backward ran on
    names = family_of(lat)
    kf = depth(plx.lattice_cache().get(xt.detach(), dk.get_coeffs().numpy()))
    return out.detach().cpu().numpy(), xt.grad.cpu().numpy(), vt.grad.cpu().numpy(), depth(lat), names, kf


@pytest.mark.parametrize("d,L", [(3, 2), (8, 3), (8, 11)])
def test_autograd_in_double_both_routes(d, L):
    """(K(x) V . G).sum().backward() in double: x.grad and V.grad of the native route (fused_backward_f64 = True) and of the
    torch route (False) under the bars of the module docstring; the two routes agree within twice the bar."""
    dk = dkernel("rbf", 1)
    taps, dtaps = dk.get_coeffs().numpy(), dk.get_deriv_coeffs().numpy()
    x = positions64("gauss1", N, d, seed=d + L, coeffs=dtaps)
    rng = np.random.default_rng(d * L)
    v, w = rng.standard_normal((N, L)), rng.standard_normal((N, L))
    want, want_gs, T, tg = reference(w, v, x, Lattice64(x, dtaps))
    fwd = Lattice64(x, taps)
    want_out, t_out = fwd.apply_staged(v), fwd.terms64(v)
    before = plx.LatticeFilterGeneral.fused_backward_f64
    res = {}
    try:
        for fused in (True, False):
            plx.lattice_cache().clear()
            res[fused] = _autograd(dk, x, v, w, fused)
    finally:
        plx.LatticeFilterGeneral.fused_backward_f64 = before
        plx.lattice_cache().clear()
    assert res[True][4] == expect(d, L), res[True][4]                 # the native route ran the new kernels ...
    assert not set(res[False][4]) & set(CHUNK + WIDE), res[False][4]  # ... and the torch route did not
    for fused, (out, gx, gv, k, _, kf) in res.items():
        assert ratio_to_bar(out, want_out.astype(LD), t_out, kf * U2, "out") <= 1.0, fused
        bar_x, bar_s = 2 * (k + 4 * (L + 1)) * U2, k * U2
        rx = ratio_to_bar(gx, want, T, bar_x, "x.grad")
        rs = ratio_to_bar(gv, want_gs.astype(LD), tg, bar_s, "V.grad")
        print(f"autograd double d={d} L={L} fused={fused}: x.grad / bar {rx:.3f}  V.grad / bar {rs:.3f}")
        assert rx <= 1.0 and rs <= 1.0, (fused, rx, rs)
        assert gx.dtype == np.float64 and gv.dtype == np.float64
    k = res[True][3]
    assert np.array_equal(res[True][0], res[False][0])                # the forward is the same call on both routes
    agree = ratio_to_bar(res[True][1], res[False][1].astype(LD), T, 2 * 2 * (k + 4 * (L + 1)) * U2, "routes")
    print(f"autograd double d={d} L={L}: native against torch route, x.grad / (2 bar) {agree:.3f}")
    assert agree <= 1.0, agree


def test_marginal_log_likelihood_gradients_agree():
    """marginal_log_likelihood(model.double(), ...).backward() at N = 2000, d = 3: the hyper-parameter gradients of the two
    routes agree to 1e-8 relative (the bar of tests/test_cg_f64_gpu.py (c), for the same reason: both solves converge to
    1e-10, what differs between the routes is rounding)."""
    import math
    n, d = 2000, 3
    x = cuda(cloud("gauss1", n, d, seed=2))
    y = torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(3), dtype=F64).cuda()
    grads, calls = {}, {True: 0, False: 0}
    before, orig = plx.LatticeFilterGeneral.fused_backward_f64, plx.Lattice.apply_backward

    def counted(self, *args, **kw):
        calls[plx.LatticeFilterGeneral.fused_backward_f64] += 1
        return orig(self, *args, **kw)

    plx.Lattice.apply_backward = counted
    try:
        for fused in (True, False):
            plx.LatticeFilterGeneral.fused_backward_f64 = fused
            plx.lattice_cache().clear()
            torch.manual_seed(0)
            model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).double().cuda()
            with torch.no_grad():
                model.raw_noise.fill_(math.log(math.expm1(1.0 - model.min_noise)))
            mll = solvers.marginal_log_likelihood(model, x, y, num_probes=4, cg_tol=1e-10, pre_size=0)
            assert mll.dtype == F64 and bool(torch.isfinite(mll))
            mll.backward()
            grads[fused] = {name: p.grad.detach().cpu().numpy().copy() for name, p in model.named_parameters()}
            for name, gr in grads[fused].items():
                assert gr.dtype == np.float64 and np.all(np.isfinite(gr)), name
    finally:
        plx.LatticeFilterGeneral.fused_backward_f64 = before
        plx.Lattice.apply_backward = orig
        plx.lattice_cache().clear()
    assert calls[True] >= 1 and calls[False] == 0, calls          # the native route was taken where it was switched on
    assert any("lengthscale" in name for name in grads[True])
    for name, a in grads[True].items():
        b = grads[False][name]
        rel = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
        print(f"marginal_log_likelihood in double, {name}.grad: native {a.ravel()[:3]}, torch {b.ravel()[:3]}, relative {rel:.2e}")
        assert rel <= 1e-8, (name, rel)


def family_report():
    lines = ["float64 position gradient against Lattice64, worst ratio to the bar per kernel family (grad_x, grad_src):"]
    for fam, (a, b, c) in sorted(WORST.items()):
        lines.append(f"  {fam[0]} | {fam[1]}: {a:.3f} {b:.3f} ({c} cases)")
    return "\n".join(lines)


def test_every_new_kernel_was_launched():
    """Every kernel name plx_backward_f64.hip can report ran in this module (run as a whole)."""
    import os
    import re
    print(family_report())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "simplex_gp_amd", "csrc", "plx_backward_f64.hip")).read()
    literals = set()
    for stmt in re.finditer(r"\bkn_f64_(?:splat|slice)\s*=([^;]*);", text):
        literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    assert literals == set(CHUNK + WIDE), literals
    assert REACHED == literals, sorted(literals - REACHED)
    for lat in (v[4] for v in _REF.values()):
        lat.close()
    _REF.clear()
