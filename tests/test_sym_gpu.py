"""The transposed and the symmetrised fp32 lattice products on the GPU (simplex_gp_amd/csrc/plx_sym.hip): plx_blur_t /
plx_apply_t, plx_blur_sym / plx_apply_sym / plx_apply_affine_sym and what is built on them.

Yardsticks: tests/sym64.Sym64 (Kt64: reversed axes with mirrored taps; Ks64 = (K64 + Kt64) / 2) on the lattices of
tests/test_sym_f64_gpu.py, and the bars of tests/sym32.py (tests/test_sym32.py shows on the CPU that plain fp32 arithmetic
meets them).

Bars, derived, not measured:
  bit contracts   torch.equal: no atomics, every sum in a fixed order; each chain of blur_dual_kernel forms the sums of
                  blur_axis_kernel, so wherever the plain blur runs that (general) family blur_sym_f32 is 0.5 * (blur +
                  blur_t_f32) to the bit; in the other families to 2^-24 (|blur| + |blur_t|) per entry;
  accuracy        per entry ENTRY * T_t for K^T, (ENTRY + 2^-24) * T_s for K_s, exactly 0 where T is 0; rel-L2 <= REL;
  adjoint         both sides are sums of fp32 outputs, each within ENTRY of its terms: 2 ENTRY sum |a| T(b);
  partial dots    a fixed-order sum of at most 1024 per-tile partials per thread-strided slot, then a 10-level tree:
                  16 * 2^-24 of the sum of their magnitudes; the dots themselves sum n fp32 products in a fixed order:
                  (n + 4) 2^-24 sum |v| |out|, the form of the fused dot's bar in plx.h;
  solve           true relative residual <= 4 x what the same batched_cg reaches on the CPU in float32 with the dense
                  matrix (the project's margin over a measured reference), and >= 10 x below the plain
                  operator's residual from the same call with the switch off.
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import solvers
from simplex_gp_amd._native import PlxError
from tests.lattice64 import cloud, entry_ratio, rel_l2
from tests.sym32 import ENTRY, ENTRY_SYM, REL, U32, ratios
from tests.sym64 import Sym64, taps_of
from tests.test_sym_f64_gpu import _Taps, operator

pytestmark = pytest.mark.gpu

F32 = torch.float32
PLX_ERR_INVALID, PLX_ERR_STATE = 1, 5
DS, ORDERS, VDS = (1, 2, 3, 8), (0, 1, 2, 3, 4), (1, 2, 3, 12, 20, 130)
CLOUDS = ("gauss1", "isolated", "dup")
GENERAL = ["blur_axis_kernel"]
DUAL = ["blur_dual_kernel"]


def _cases():
    """(cloud, n, d, order, lopsided, vd, aligned, lattice_rows).  Every (d, order) pair twice with the widths, tap kinds,
    clouds, sizes, alignments and row orders rotating through it; then the cases the bit contract against the plain blur
    must not miss -- vd = 1 at orders 0 and 4, vd = 20 at every order (the general family) -- at an even d (the middle
    launch shares its ids) and an odd one, and every width at d = 2, order 3."""
    out = []
    i = 0
    for a, d in enumerate(DS):
        for b, order in enumerate(ORDERS):
            for rep in range(2):
                vd = VDS[(a + b + 3 * rep + (i // 5) % 2) % len(VDS)]
                out.append((CLOUDS[i % 3], (64, 300)[(i // 3 + rep) % 2], d, order, i % 2 == 1, vd, (i // 2) % 2 == 0,
                            (i // 4) % 2 == 1))
                i += 1
    for order in ORDERS:
        out.append(("gauss1", 701, 2 if order % 2 else 3, order, True, 20, order % 2 == 0, order % 2 == 1))
    for order in (0, 4):
        out.append(("gauss1", 701, 2, order, True, 1, True, order == 4))
    for vd in VDS:
        out.append(("gauss1", 300, 2, 3, True, vd, vd % 2 == 0, vd % 3 == 0))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()
IDS = [f"{c}-n{n}-d{d}-o{o}-{'lop' if l else 'sym'}-vd{vd}-{'al' if al else 'off'}-{'lrows' if lr else 'crows'}"
       for c, n, d, o, l, vd, al, lr in CASES]
MUST_BE_GENERAL = [c for c in CASES if (c[5] == 1 and c[3] in (0, 4)) or c[5] == 20]
_LATS = {}
_WORST = {"K^T entry": 0.0, "K_s entry": 0.0, "K^T rel": 0.0, "K_s rel": 0.0, "other families": 0.0}


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print("\nworst ratios of tests/test_sym_gpu.py:", {k: f"{v:.2e}" for k, v in _WORST.items()})


def test_case_list_holds_the_general_family_cases():
    have = {(c[5], c[3]) for c in MUST_BE_GENERAL}
    assert {(1, 0), (1, 4)} <= have and {(20, o) for o in ORDERS} <= have
    assert {c[5] for c in CASES} == set(VDS) and {c[2] for c in CASES} == set(DS) and {c[3] for c in CASES} == set(ORDERS)
    assert {c[6] for c in CASES} == {True, False} and {c[7] for c in CASES} == {True, False}
    assert max(c[1] for c in CASES) <= 701


def cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def gpu_lattice(kind, n, d, order, lop):
    key = (kind, n, d, order, lop)
    if key not in _LATS:
        x, _, taps = operator(*key)
        _LATS[key] = plx.Lattice().build(cuda(x), taps)
    return _LATS[key]


def placed(rows, vd, aligned, fill=None):
    """A contiguous [rows, vd] float32 CUDA tensor whose data pointer is 16-byte aligned, or that plus one float."""
    buf = torch.empty(rows * vd + 4, dtype=F32, device="cuda")
    off = 0 if aligned else 1
    t = buf[off:off + rows * vd].view(rows, vd)
    assert t.data_ptr() % 16 == (0 if aligned else 4)
    if fill is not None:
        t.copy_(fill)
    else:
        t.fill_(float("nan"))
    return t


def note(key, value):
    _WORST[key] = max(_WORST[key], float(value))


@pytest.mark.parametrize("kind,n,d,order,lop,vd,aligned,lrows", CASES, ids=IDS)
def test_transposed_and_symmetrised_products(kind, n, d, order, lop, vd, aligned, lrows):
    case = (kind, n, d, order, lop, vd, aligned, lrows)
    label = IDS[CASES.index(case)]
    x, op, taps = operator(kind, n, d, order, lop)
    lat = gpu_lattice(kind, n, d, order, lop)
    assert lat.m == op.m and lat.order == order and lat.d == d
    v = np.random.default_rng(vd + 11 * d).standard_normal((n, vd)).astype(np.float32)
    if kind == "isolated":
        v[::2] = 0.0                                   # points no other point reaches: T = 0 there, and so must the products be
    lat.set_lattice_row_order(lrows)
    try:
        to_rows = lat.to_lattice_order if lrows else (lambda t: t)
        from_rows = lat.from_lattice_order if lrows else (lambda t: t)
        src = placed(n, vd, aligned, to_rows(cuda(v)))
        plain = lat.apply(src).clone()
        plain_names = lat.stage_kernels()

        # the blurs, from the staged results
        V = lat.splat(src)
        b = lat.blur(V.clone(), vd=vd).clone()
        family = lat.stage_kernels()["blur_axis"]
        bt = lat.blur_t_f32(V.clone(), vd=vd).clone()
        assert lat.sym_kernels_f32()["blur"] == GENERAL
        bs = lat.blur_sym_f32(V.clone(), vd=vd).clone()
        assert lat.sym_kernels_f32()["blur"] == DUAL
        assert bs.shape == b.shape == bt.shape
        assert torch.equal(lat.blur_t_f32(V.clone(), vd=vd), bt) and torch.equal(lat.blur_sym_f32(V.clone(), vd=vd), bs)
        mean = 0.5 * (b + bt)
        if case in MUST_BE_GENERAL:
            # the bit contract cannot be skipped silently: the cases it is promised for do run the general family
            assert family == GENERAL, (label, family)
        if family == GENERAL:
            assert torch.equal(bs, mean), (label, "blur_sym_f32 is not 0.5 (blur + blur_t_f32) to the bit")
        else:
            gap = (bs.double() - mean.double()).abs()
            allow = U32 * (b.double().abs() + bt.double().abs())
            worst = float((gap / allow.clamp_min(1e-300)).max()) if bool((allow > 0).any()) else 0.0
            print(f"{label}: family {family}: max |blur_sym - 0.5 (blur + blur_t)| / (|blur| + |blur_t|) = {worst * U32:.2e} "
                  f"(bar {U32:.2e})")
            note("other families", worst * U32)
            assert bool((gap <= allow).all()), (label, family, worst)

        # the products against their staged forms, twice, with no allocation the second time
        got_t = lat.apply_t_f32(src, out=placed(n, vd, aligned)).clone()
        names_t = lat.sym_kernels_f32()
        got_s = lat.apply_sym_f32(src, out=placed(n, vd, aligned)).clone()
        names_s = lat.sym_kernels_f32()
        assert names_t["blur"] == GENERAL and names_t["splat"] and names_t["slice"], names_t
        assert names_s["blur"] == DUAL and names_s["splat"] and names_s["slice"], names_s
        bytes1 = lat.device_bytes
        assert torch.equal(lat.apply_t_f32(src, out=placed(n, vd, aligned)), got_t), (label, "apply_t_f32 not deterministic")
        assert torch.equal(lat.apply_sym_f32(src, out=placed(n, vd, aligned)), got_s), (label, "apply_sym_f32 not deterministic")
        assert lat.device_bytes == bytes1, (label, "the second call of a width moved plx_device_bytes")
        assert torch.equal(lat.slice(bt, out=placed(n, vd, aligned), vd=vd), got_t), (label, "apply_t_f32 != slice(blur_t(splat))")
        assert torch.equal(lat.slice(bs, out=placed(n, vd, aligned), vd=vd), got_s), (label, "apply_sym_f32 != slice(blur_sym(splat))")
        one = torch.tensor([1.0, 0.0], device="cuda")
        aff = lat.apply_affine_sym_f32(src, one, out=placed(n, vd, aligned))
        assert torch.equal(aff, got_s), (label, "apply_affine_sym_f32 with (1, 0) differs from apply_sym_f32")
        if 2 <= vd <= 256:
            out_d, dot = lat.apply_affine_sym_f32(src, one, out=placed(n, vd, aligned), want_dot=True)
            dot = dot.clone()
            out_p, work, tiles = lat.apply_affine_sym_f32(src, one, out=placed(n, vd, aligned), want_dot="partial")
            assert torch.equal(out_d, got_s) and torch.equal(out_p, got_s) and dot.shape == (vd,)
            stride = plx.Lattice.values_stride(vd)
            assert tiles == int(nv.lib().plx_affine_dot_tiles(lat._h, vd)) and work.numel() >= tiles * stride
            part = work[:tiles * stride].view(tiles, stride)[:, :vd].double()
            assert bool(((part.sum(0) - dot.double()).abs() <= 16 * U32 * part.abs().sum(0)).all()), label
            exact_dot = (src.double() * got_s.double()).sum(0)
            # (the dot is the plain slice kernel's: n products summed in fp32 in a fixed order, the bar of the fused dot)
            assert bool(((dot.double() - exact_dot).abs() <= (n + 4) * U32 * (src.double() * got_s.double()).abs().sum(0)).all())
        # the plain product and what it reports are untouched
        assert lat.stage_kernels() == plain_names and torch.equal(lat.apply(src), plain)

        # accuracy against Kt64 / Ks64
        gt, gs = from_rows(got_t).cpu().numpy(), from_rows(got_s).cpu().numpy()
    finally:
        lat.set_lattice_row_order(False)
    et, es, Tt, Ts = ratios(op, v, gt, gs)
    v64 = v.astype(np.float64)
    rt, rs = rel_l2(gt, op.kt.apply_staged(v64)), rel_l2(gs, op.apply_staged(v64))
    print(f"{label}: K^T entry {et:.2e} (bar {ENTRY:.2e}) rel-L2 {rt:.2e}; K_s entry {es:.2e} (bar {ENTRY_SYM:.2e}) rel-L2 {rs:.2e} "
          f"(bar {REL:.2e})")
    note("K^T entry", et); note("K_s entry", es); note("K^T rel", rt); note("K_s rel", rs)
    assert et <= ENTRY and es <= ENTRY_SYM, (label, et, es)
    assert rt <= REL and rs <= REL, (label, rt, rs)
    if kind == "isolated":
        zero = (Ts == 0).all(axis=1) & (Tt == 0).all(axis=1)
        assert zero.sum() >= n // 2 - 1
        assert bool((gs[zero] == 0).all()) and bool((gt[zero] == 0).all()), label


ADJOINT = [("gauss1", 300, 3, 2, True, 3), ("dup", 300, 8, 1, True, 2), ("gauss1", 64, 2, 4, True, 1),
           ("gauss1", 300, 1, 3, False, 12), ("gauss1", 300, 2, 3, True, 20)]


@pytest.mark.parametrize("kind,n,d,order,lop,vd", ADJOINT)
def test_adjoint_identities(kind, n, d, order, lop, vd):
    x, op, taps = operator(kind, n, d, order, lop)
    lat = gpu_lattice(kind, n, d, order, lop)
    rng = np.random.default_rng(d + vd)
    a, b = rng.standard_normal((n, vd)).astype(np.float32), rng.standard_normal((n, vd)).astype(np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    at, bt = cuda(a), cuda(b)
    bar = 2 * ENTRY * float((np.abs(a64) * op.k.terms64(b64)).sum())
    lhs = float((lat.apply_t_f32(at).cpu().numpy().astype(np.float64) * b64).sum())
    rhs = float((a64 * lat.apply(bt).cpu().numpy().astype(np.float64)).sum())
    print(f"<K^T a, b> - <a, K b> = {lhs - rhs:.2e} (bar {bar:.2e})")
    assert abs(lhs - rhs) <= bar
    bar_s = 2 * ENTRY * float((np.abs(a64) * op.terms64(b64)).sum())
    lhs = float((lat.apply_sym_f32(at).cpu().numpy().astype(np.float64) * b64).sum())
    rhs = float((a64 * lat.apply_sym_f32(bt).cpu().numpy().astype(np.float64)).sum())
    print(f"<K_s a, b> - <a, K_s b> = {lhs - rhs:.2e} (bar {bar_s:.2e})")
    assert abs(lhs - rhs) <= bar_s


def test_rebuild_on_the_same_object():
    """The work planes follow the build: another build on the same object (other points, other dimension, other order) is
    served from its own tables, and going back gives the first result bit for bit."""
    lat = plx.Lattice()
    outs = []
    for key in (("gauss1", 300, 3, 2, True), ("gauss1", 300, 8, 1, True), ("gauss1", 300, 3, 2, True)):
        x, op, taps = operator(*key)
        lat.build(cuda(x), taps)
        for vd in (1, 3):
            v = np.random.default_rng(vd).standard_normal((op.n, vd)).astype(np.float32)
            got = lat.apply_sym_f32(cuda(v))
            et, es, _, _ = ratios(op, v, lat.apply_t_f32(cuda(v)).cpu().numpy(), got.cpu().numpy())
            assert et <= ENTRY and es <= ENTRY_SYM, (key, vd, et, es)
            outs.append(got.clone())
    assert torch.equal(outs[0], outs[4]) and torch.equal(outs[1], outs[5])
    lat.close()


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def test_refusals():
    n, d = 300, 3
    taps = taps_of(1, True)
    x = cuda(cloud("gauss1", n, d, seed=1, coeffs=taps))
    v = cuda(np.random.default_rng(5).standard_normal((n, 2)))
    lat = plx.Lattice().build(x, taps)
    L = nv.lib()
    # float64 tensors go to the float64 methods
    ss64 = torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda")
    vals64 = lat.new_values(2, torch.float64)
    for call, name in ((lambda: lat.apply_t_f32(v.double()), "apply_t"), (lambda: lat.apply_sym_f32(v.double()), "apply_sym"),
                       (lambda: lat.blur_t_f32(vals64, vd=2), "blur_t"), (lambda: lat.blur_sym_f32(vals64, vd=2), "blur_sym"),
                       (lambda: lat.apply_affine_sym_f32(v.double(), ss64), "apply_affine")):
        with pytest.raises(TypeError, match=name):
            call()
    # vd = 0, NULL pointers, an aliased d_out for the affine call: PLX_ERR_INVALID, before any GPU work
    out, ss = torch.empty_like(v), torch.tensor([1.0, 0.0], device="cuda")
    for fn in (L.plx_apply_t, L.plx_apply_sym):
        assert fn(lat._h, _ptr(v), 0, _ptr(out), None) == PLX_ERR_INVALID
        assert fn(lat._h, None, 2, _ptr(out), None) == PLX_ERR_INVALID
        assert fn(lat._h, _ptr(v), 2, None, None) == PLX_ERR_INVALID
        assert fn(None, _ptr(v), 2, _ptr(out), None) == PLX_ERR_INVALID
    assert L.plx_apply_affine_sym(lat._h, _ptr(v), 0, _ptr(out), _ptr(ss), None, None, None) == PLX_ERR_INVALID
    assert L.plx_apply_affine_sym(lat._h, _ptr(v), 2, _ptr(out), None, None, None, None) == PLX_ERR_INVALID
    assert L.plx_apply_affine_sym(lat._h, _ptr(v), 2, _ptr(v), _ptr(ss), None, None, None) == PLX_ERR_INVALID
    assert b"alias" in L.plx_last_error()
    assert L.plx_apply_affine_sym(lat._h, _ptr(v), 2, _ptr(out), _ptr(ss), _ptr(ss), None, None) == PLX_ERR_INVALID   # a dot without work
    v1 = cuda(np.ones((n, 1)))
    assert L.plx_apply_affine_sym(lat._h, _ptr(v1), 1, _ptr(torch.empty_like(v1)), _ptr(ss), None, _ptr(out), None) == PLX_ERR_INVALID
    assert b"2..256" in L.plx_last_error()
    # the value planes: overlap, misalignment
    vals = lat.new_values(2)
    need = int(L.plx_blur_sym_work_floats(lat._h, 2))
    work = torch.empty(need + 4, dtype=F32, device="cuda")
    res, flag = ctypes.c_void_p(0), ctypes.c_int(0)
    assert L.plx_blur_sym(lat._h, _ptr(vals), _ptr(work), 0, ctypes.byref(res), None) == PLX_ERR_INVALID
    assert L.plx_blur_sym(lat._h, _ptr(vals), None, 2, ctypes.byref(res), None) == PLX_ERR_INVALID
    assert L.plx_blur_sym(lat._h, _ptr(vals), _ptr(work), 2, None, None) == PLX_ERR_INVALID
    assert L.plx_blur_sym(lat._h, _ptr(vals), _ptr(vals), 2, ctypes.byref(res), None) == PLX_ERR_INVALID
    assert b"overlap" in L.plx_last_error()
    assert L.plx_blur_sym(lat._h, _ptr(work, 16), _ptr(work), 2, ctypes.byref(res), None) == PLX_ERR_INVALID      # values inside work
    assert b"overlap" in L.plx_last_error()
    assert L.plx_blur_sym(lat._h, _ptr(vals), _ptr(work, 4), 2, ctypes.byref(res), None) == PLX_ERR_INVALID       # work off by one float
    assert b"aligned" in L.plx_last_error()
    big = torch.empty(2 * vals.numel() + 8, dtype=F32, device="cuda")
    assert L.plx_blur_sym(lat._h, _ptr(big, 4), _ptr(work), 2, ctypes.byref(res), None) == PLX_ERR_INVALID
    assert b"aligned" in L.plx_last_error()
    assert L.plx_blur_t(lat._h, _ptr(vals), _ptr(vals), 2, ctypes.byref(flag), None) == PLX_ERR_INVALID
    assert L.plx_blur_t(lat._h, _ptr(big), _ptr(big, 16), 2, ctypes.byref(flag), None) == PLX_ERR_INVALID         # overlapping planes
    assert b"overlap" in L.plx_last_error()
    assert L.plx_blur_t(lat._h, _ptr(vals), _ptr(work, 4), 2, ctypes.byref(flag), None) == PLX_ERR_INVALID
    assert L.plx_blur_t(lat._h, _ptr(vals), _ptr(work), 0, ctypes.byref(flag), None) == PLX_ERR_INVALID
    assert L.plx_blur_t(lat._h, _ptr(vals), _ptr(work), 2, None, None) == PLX_ERR_INVALID
    # a single column needs no alignment
    vals1, work1 = lat.new_values(1), torch.empty(int(L.plx_blur_sym_work_floats(lat._h, 1)) + 1, dtype=F32, device="cuda")
    vals1.normal_()
    assert L.plx_blur_sym(lat._h, _ptr(vals1), _ptr(work1, 4), 1, ctypes.byref(res), None) == 0
    # the work space: -1 for vd < 1 or an unbuilt lattice, min(d + 1, 3) planes
    assert L.plx_blur_sym_work_floats(lat._h, 0) == -1
    assert L.plx_blur_sym_work_floats(lat._h, 3) == 3 * lat.m * plx.Lattice.values_stride(3)
    fresh = plx.Lattice()
    assert L.plx_blur_sym_work_floats(fresh._h, 2) == -1
    assert L.plx_apply_sym(fresh._h, _ptr(v), 2, _ptr(out), None) == PLX_ERR_STATE
    assert L.plx_apply_t(fresh._h, _ptr(v), 2, _ptr(out), None) == PLX_ERR_STATE
    fresh.close()
    lat.close()
    # a sharded lattice
    lat = plx.Lattice().build(x, taps, shard=(0, 2))
    own = lat.n_owned
    for call in (lambda: lat.apply_t_f32(v[:own]), lambda: lat.apply_sym_f32(v[:own]), lambda: lat.apply_affine_sym_f32(v[:own], ss)):
        with pytest.raises(PlxError) as err:
            call()
        assert err.value.code == PLX_ERR_STATE and "shard" in str(err.value)
    lat.close()
    # a build that replayed the reference's table growth: its neighbour table is not symmetric
    nv.check(L.plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        lat = plx.Lattice().build(x, taps)
    finally:
        nv.check(L.plx_tune(b"reference_growth", 0), "plx_tune")
    assert lat.reference_growth_info()["replayed"]
    for call in (lambda: lat.apply_t_f32(v), lambda: lat.apply_sym_f32(v), lambda: lat.apply_affine_sym_f32(v, ss),
                 lambda: lat.blur_t_f32(lat.new_values(2), vd=2), lambda: lat.blur_sym_f32(lat.new_values(2), vd=2)):
        with pytest.raises(PlxError) as err:
            call()
        assert err.value.code == PLX_ERR_STATE and "reference_growth" in str(err.value)
    lat.close()


def test_first_call_under_capture_is_refused():
    rng = np.random.default_rng(3)
    n, d = 2000, 3
    lat = plx.Lattice().build(cuda(rng.standard_normal((n, d))), taps_of(1, True))
    v = cuda(rng.standard_normal((n, 4)))
    out = torch.empty_like(v)
    lat.apply(v)                                            # the plain workspace exists; the two further planes do not
    before = lat.device_bytes
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(PlxError, match="captured") as err:
        with torch.cuda.graph(graph, stream=s):
            lat.apply_sym_f32(v, out=out)
    assert err.value.code == PLX_ERR_STATE and lat.device_bytes == before
    del graph
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        eager = lat.apply_sym_f32(v, out=out).clone()
        first = lat.device_bytes
        assert first >= before + 2 * lat.m * 4 * 4
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        out.zero_()
        with torch.cuda.graph(graph, stream=s):
            lat.apply_sym_f32(v, out=out)
        graph.replay()
        s.synchronize()
        assert torch.equal(out, eager) and lat.device_bytes == first
    torch.cuda.synchronize()
    lat.close()


class _Identity:
    """A preconditioner that is not the native one: khat_solve keeps the caller's row order for it."""

    def solve(self, R):
        return R.clone()


def _solve_model(d):
    """LatticeGP whose operator is 1 * K + 0.1 I with the taps [0.5, 1, 0.5] on x / 1."""
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).cuda()
    inv_softplus = lambda y: float(np.log(np.expm1(y)))        # noqa: E731
    with torch.no_grad():
        model.kernel.raw_lengthscale.fill_(inv_softplus(1.0))
        model.raw_outputscale.fill_(inv_softplus(1.0))
        model.raw_noise.fill_(inv_softplus(0.1 - model.min_noise))
    model.kernel.dkernel_fn._forward_coeffs = torch.from_numpy(taps_of(1, False))
    return model


def test_solve_on_the_symmetrised_operator():
    """khat_solve with symmetric_f32 on (n = 300, d = 2, cloud gauss1, taps [0.5, 1, 0.5], noise 0.1, three randn columns,
    max_iter 400, tol 1e-6): the true relative residual, formed in float64 from Sym64.matrix(), is at most 4 x what the same
    batched_cg reaches on the CPU in float32 with the dense matrix, and at least 10 x below the plain operator's residual
    from the same call with the switch off.  Measured on the CPU alone (the reference of both conditions): K_s 1.4e-5 in 68
    iterations, K 1.7e-2 after 400.  The caller-order branch (a foreign preconditioner) is held to the first condition."""
    n, d, tol = 300, 2, 1e-6
    x32 = cloud("gauss1", n, d, seed=6, coeffs=taps_of(1, False))
    model = _solve_model(d)
    assert solvers.LatticeGP.symmetric_f32 is False
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(0))
    Bn = B.numpy().astype(np.float64)
    try:
        with torch.no_grad():
            xg = cuda(x32)
            ref = (xg / model.kernel.lengthscale).cpu().numpy()       # the positions the lattice is built on
            s, noise = float(model.outputscale.detach()), float(model.noise.detach())
        op = Sym64(ref, taps_of(1, False))
        A_s, A_k = s * op.matrix() + noise * np.eye(n), s * op.k.matrix() + noise * np.eye(n)
        true_res = lambda A, X: float(np.linalg.norm(A @ X.double().cpu().numpy() - Bn) / np.linalg.norm(Bn))      # noqa: E731
        # the reference: the same iteration on the CPU in float32 with the dense matrices
        A32 = torch.from_numpy(A_s.astype(np.float32))
        Xc, ic = solvers.batched_cg(lambda V: A32 @ V, B.clone(), max_iter=400, tol=tol)
        res_cpu = true_res(A_s, Xc)
        K32 = torch.from_numpy(A_k.astype(np.float32))
        Xk, _ = solvers.batched_cg(lambda V: K32 @ V, B.clone(), max_iter=400, tol=tol)
        res_cpu_plain = true_res(A_k, Xk)
        assert res_cpu_plain >= 10 * res_cpu, (res_cpu, res_cpu_plain)      # the reference alone meets the second condition
        # the plain operator, switch off
        Xp, ip = model.khat_solve(xg, B.cuda(), max_iter=400, tol=tol)
        res_plain = true_res(A_k, Xp)
        model.symmetric_f32 = True
        Xs, info = model.khat_solve(xg, B.cuda(), max_iter=400, tol=tol)
        res = true_res(A_s, Xs)
        Xo, io = model.khat_solve(xg, B.cuda(), max_iter=400, tol=tol, precond=_Identity())
        res_caller = true_res(A_s, Xo)
        print(f"solve n = {n}, d = {d}, s = {s:.6f}, noise = {noise:.6f}: K_s true relative residual {res:.2e} in "
              f"{info['iterations']} iterations (CPU fp32 dense: {res_cpu:.2e} in {ic['iterations']}); caller-order branch "
              f"{res_caller:.2e} in {io['iterations']}; plain K {res_plain:.2e} in {ip['iterations']} (CPU: {res_cpu_plain:.2e})")
        assert Xs.dtype == F32 and Xs.shape == (n, 3)
        assert res <= 4 * res_cpu, (res, res_cpu)
        assert res_caller <= 4 * res_cpu, (res_caller, res_cpu)
        assert 10 * res <= res_plain, (res, res_plain)
    finally:
        plx.lattice_cache().clear()


def test_khat_in_lattice_rows_follows_the_switch():
    n, d = 300, 3
    x = cuda(np.random.default_rng(2).standard_normal((n, d)))
    V = cuda(np.random.default_rng(3).standard_normal((n, 4)))
    try:
        model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).cuda()
        with torch.no_grad():
            s, noise = model.outputscale, model.noise
            with model.khat_in_lattice_rows(x) as (mm, to_rows, from_rows):
                plain = from_rows(mm(to_rows(V))).clone()
            model.symmetric_f32 = True
            with model.khat_in_lattice_rows(x) as (mm, to_rows, from_rows):
                got = from_rows(mm(to_rows(V))).clone()
            ref = x / model.kernel.lengthscale.detach()
            lat = plx.lattice_cache().get(ref.contiguous(), model.kernel.dkernel_fn.get_coeffs())
            assert lat.lattice_rows is False
            ks = lat.apply_sym_f32(V)
            want = s * ks + noise * V
            # both sides are fp32 evaluations of s K_s V + sigma^2 V, each within ENTRY_SYM of the size of its terms (taps
            # and weights are non-negative: K_s |V| is that size); the affine tail adds roundings of the same terms
            terms = s * lat.apply_sym_f32(V.abs()) + noise * V.abs()
            assert bool(((got - want).abs() <= 2 * (ENTRY_SYM + 2 * U32) * terms).all())
            assert not torch.allclose(got, plain, rtol=0, atol=1e-4)
            assert torch.allclose(plain, s * lat.apply(V) + noise * V, rtol=0, atol=1e-5)
    finally:
        plx.lattice_cache().clear()


def test_exact_adjoint_of_the_source_gradient():
    """Lopsided taps, n = 64: with exact_adjoint_f32 on grad_source is apply_t_f32(g) bit for bit and stays within the K^T
    bar of the float64 Kt64 g; with the switch off it is K g, as it was."""
    n, d, vd = 64, 3, 2
    taps = taps_of(1, True)
    fn = _Taps(taps, np.array([-0.5, 0.0, 0.5], np.float32))
    xn = cloud("gauss1", n, d, seed=2, coeffs=taps)
    x = cuda(xn)
    gn = np.random.default_rng(1).standard_normal((n, vd)).astype(np.float32)
    g = cuda(gn)
    before = plx.LatticeFilterGeneral.exact_adjoint_f32
    grads = {}
    try:
        for on in (False, True):
            plx.LatticeFilterGeneral.exact_adjoint_f32 = on
            src = cuda(np.random.default_rng(0).standard_normal((n, vd))).requires_grad_(True)
            (plx.LatticeFilterGeneral.apply(src, x, fn) * g).sum().backward()
            grads[on] = src.grad.clone()
        lat = plx.lattice_cache().get(x, taps)
        assert torch.equal(grads[True], lat.apply_t_f32(g))
        assert torch.equal(grads[False], lat.apply(g))
        assert not torch.equal(grads[True], grads[False])
        op = Sym64(xn, taps)
        et, _, _, _ = ratios(op, gn, grads[True].cpu().numpy(), None)
        print(f"grad_source against Kt64 g: entry {et:.2e} (bar {ENTRY:.2e})")
        assert et <= ENTRY
    finally:
        plx.LatticeFilterGeneral.exact_adjoint_f32 = before
        plx.lattice_cache().clear()
    assert before is False


def test_exact_adjoint_with_a_position_gradient():
    """The branches that return the derivative-tap filter of g: with the switch on grad_source is K^T g with the forward taps
    there too, and the position gradient is what it was.  vd = 2: the three-call position gradient; vd = 16, d = 3: the
    fused one (Lattice.backward_fusable)."""
    n, d = 300, 3
    dk = plx.DiscretizedKernelFN(plx.rbf, 1)
    taps = dk.get_coeffs().numpy()
    xn = cloud("gauss1", n, d, seed=4, coeffs=taps)
    before = plx.LatticeFilterGeneral.exact_adjoint_f32
    try:
        for vd in (2, 16):
            assert plx.Lattice.backward_fusable(vd, d) is (vd == 16)
            g = cuda(np.random.default_rng(1).standard_normal((n, vd)))
            grads = {}
            for on in (False, True):
                plx.LatticeFilterGeneral.exact_adjoint_f32 = on
                x = cuda(xn).requires_grad_(True)
                src = cuda(np.random.default_rng(0).standard_normal((n, vd))).requires_grad_(True)
                (plx.LatticeFilterGeneral.apply(src, x, dk) * g).sum().backward()
                grads[on] = (src.grad.clone(), x.grad.clone())
            lat = plx.lattice_cache().get(cuda(xn), taps)
            assert torch.equal(grads[True][0], lat.apply_t_f32(g))
            assert torch.equal(grads[True][1], grads[False][1])
            assert not torch.equal(grads[True][0], grads[False][0])
    finally:
        plx.LatticeFilterGeneral.exact_adjoint_f32 = before
        plx.lattice_cache().clear()
