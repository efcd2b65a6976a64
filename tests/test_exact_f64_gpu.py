"""The float64 exact kernel MVM and its position gradient (plx_exact_f64.hip) on the GPU: the C ABI at every
instantiation against longdouble references under derived bars, and the Python surface on doubles.

C ABI.  One pytest case is one group of exact_f64.CASES: a (kind, profile, DP) with both ends of the d range, t at both
ends of every TC and with one to three column blocks, n1 around the 256-row workgroup, n2 around the 64-row LDS tile, the
ragged two-slice split, and the data kinds in rotation (a cloud, the cloud shifted by 30, coincident points, a far row),
every value off the fp32 grid.  Every device array has exactly the stated size, starts at an odd element offset in its
allocation and is followed by sentinels; the workspace is exactly plx_exact_work_bytes_f64.  Inputs come back
bit-unchanged, a second call on the used workspace is bit-equal, the slabs of a split call are all written, an empty
slice's as zeros.  Every entry must satisfy |got - want| <= bar T with exact_f64.bar, which counts the roundings an entry
can see, (TILE + DP + C + tiles + splits) 2^-53: derived in exact_f64's docstring, not measured.  Every ratio is printed
(as a share of its bar too) before anything is asserted; PLX_EXACT_F64_REPORT=<file> writes the worst ratio per family.

The cap shape (exact_f64.SPLIT_CAP: 127 slices, set by the 16 MiB workspace cap) needs about 1e9 multiply-adds for a
reference of all its entries, whatever the shape: the cap itself forces that.  It is judged two ways instead.  EVERY entry
by a bit contract: the split call equals, bit for bit, the host's in-order float64 sum of one direct call per slice (each
on that slice's rows of x2 and v, each with plx_exact_splits_f64 == 1).  And NUMERICALLY, against longdouble, rows 0, 1,
255 and 256 ONLY (both workgroups and the dead-lane boundary): those four rows are all that is judged numerically for that
one shape.  Every other case is judged on every entry.

test_every_family_was_reached fails if one of the 224 instantiations or a required slab path did not run: run the module
whole."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from tests import exact_f64 as xf
from tests.gpubuf import Buf, _bits_equal, check_buffers

pytestmark = pytest.mark.gpu

F64 = torch.float64
DEV = "cuda"
WORST = {}               # family (kind, profile, DP, TC, path) -> (worst ratio, worst ratio / its bar)
OFFSETS = dict(x1=1, x2=3, v=5, g=7, out=3, work=1)      # doubles into the allocation: nothing may assume 16-byte alignment


@pytest.fixture(scope="module")
def lib():
    from simplex_gp_amd import _native as nv
    assert torch.cuda.is_available()
    assert nv.has_symbols(*plx.exact.F64_SYMBOLS)
    return nv.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, c, X1, X2, G, V, out, work, work_bytes, n2=None):
    prof = xf.PROFILES.index(c.profile)
    n2 = c.n2 if n2 is None else n2
    if c.kind == "mvm":
        rc = lib.plx_exact_mvm_f64(X1.ptr, c.n1, X2.ptr, n2, c.d, prof, V.ptr, c.t, out.ptr, work.ptr, work_bytes, stream())
    else:
        rc = lib.plx_exact_grad_f64(X1.ptr, c.n1, X2.ptr, n2, c.d, prof, G.ptr, V.ptr, c.t, out.ptr, work.ptr, work_bytes,
                                    stream())
    assert rc == 0, (c, rc, lib.plx_last_error())
    torch.cuda.synchronize()


def run_call(lib, c, data):
    """The call on guarded buffers, twice; what every case checks.  Returns (got [n1][width], splits, the buffers)."""
    splits = lib.plx_exact_splits_f64(c.n1, c.n2, c.d, c.t)
    work_bytes = lib.plx_exact_work_bytes_f64(c.n1, c.n2, c.d, c.t)
    assert splits >= 1 and work_bytes > 0 and work_bytes % 8 == 0
    width = c.t if c.kind == "mvm" else c.d
    X1, X2, V = (Buf(data[k], offset=OFFSETS[k], dtype=F64) for k in ("x1", "x2", "v"))
    G = Buf(data["g"], offset=OFFSETS["g"], dtype=F64) if c.kind == "grad" else None
    inputs = [b for b in (X1, X2, V, G) if b is not None]
    out = Buf(count=c.n1 * width, offset=OFFSETS["out"], dtype=F64)
    again = Buf(count=c.n1 * width, offset=OFFSETS["out"], dtype=F64)
    work = Buf(count=work_bytes // 8, offset=OFFSETS["work"], dtype=F64)            # sentinels throughout
    call(lib, c, X1, X2, G, V, out, work, work_bytes)
    check_buffers(inputs, [out, work])
    if splits > 1:
        used = splits * c.n1 * width
        assert 8 * used <= work_bytes, (c, splits)
        slabs = work.cpu()[:used].reshape(splits, c.n1 * width)
        chunk = -(-c.n2 // splits)
        empty = [s for s in range(splits) if s * chunk >= c.n2]
        assert not bool((slabs == work.sent).any()), ("a slab entry was never written", c)
        assert all(bool((slabs[s] == 0).all()) for s in empty), ("the slab of an empty slice is not zero", c)
    call(lib, c, X1, X2, G, V, again, work, work_bytes)
    check_buffers(inputs, [again, work])
    got = out.cpu()
    assert got.dtype == F64 and _bits_equal(got, again.cpu()), ("two identical calls differ", c)
    return got.numpy().reshape(c.n1, width), splits, (X1, X2, G, V)


def judge(c, data, got, splits, rows=None):
    """|got - want| / T over the entries (of `rows` only, where given) and the derived bar of the call"""
    x1 = data["x1"] if rows is None else data["x1"][list(rows)]
    if c.kind == "mvm":
        want, T = xf.mvm_ld(x1, data["x2"], data["v"], c.profile)
        floor = xf.mvm_floor(c.n2, data["v"])
    else:
        g = data["g"] if rows is None else data["g"][list(rows)]
        want, T = xf.grad_ld(x1, data["x2"], g, data["v"], c.profile)
        floor = xf.grad_floor(data["x1"], data["x2"], data["g"], data["v"])
    ratio = xf.entry_ratio(got if rows is None else got[list(rows)], want, T, floor)
    bar = xf.bar(c.kind, c.d, c.t, c.n2, splits)
    fam = xf.family(c.kind, c.profile, c.d, c.t, splits)
    old = WORST.get(fam, (0.0, 0.0))
    WORST[fam] = (max(old[0], ratio), max(old[1], ratio / bar))
    print(f"{ratio:9.2e}  bar {bar:9.2e}  {ratio / bar:5.3f} of it  {'|'.join(map(str, fam))}  d={c.d} t={c.t} n1={c.n1} "
          f"n2={c.n2} {c.data} splits={splits}" + ("" if rows is None else f" rows={tuple(rows)}"))
    return ratio, bar


@pytest.mark.parametrize("group", xf.GROUPS)
def test_exact_f64_against_longdouble(lib, group):
    """every case of the group, every entry; the figures are printed before anything is asserted on them"""
    cases = [c for c in xf.CASES if c.group == group]
    results = []
    for c in cases:
        data = xf.make_data(c)
        got, splits, _ = run_call(lib, c, data)
        results.append(judge(c, data, got, splits))
    for c, (ratio, bar) in zip(cases, results):
        assert ratio <= bar, (c, ratio, bar)


@pytest.mark.parametrize("c", xf.CAP_CASES, ids=lambda c: c.group)
def test_cap_shape_by_bit_contract_and_four_rows(lib, c):
    """The split count set by the 16 MiB cap.  Every entry: the split call is bit-equal to the host's in-order float64 sum
    of one direct call per slice.  Numerically only rows 0, 1, 255 and 256 are judged against longdouble (module
    docstring): a reference of every entry costs ~1e9 multiply-adds at any shape the cap binds."""
    data = xf.make_data(c)
    got, splits, (X1, _, G, _) = run_call(lib, c, data)
    assert splits == xf.SPLIT_CAP[4]
    ratio, bar = judge(c, data, got, splits, rows=xf.CAP_ROWS)
    width = c.t if c.kind == "mvm" else c.d
    chunk = -(-c.n2 // splits)
    total = None
    for s in range(splits):
        j0, j1 = min(c.n2, s * chunk), min(c.n2, (s + 1) * chunk)
        assert j1 > j0 and lib.plx_exact_splits_f64(c.n1, j1 - j0, c.d, c.t) == 1
        wb = lib.plx_exact_work_bytes_f64(c.n1, j1 - j0, c.d, c.t)
        X2s, Vs = Buf(data["x2"][j0:j1], offset=OFFSETS["x2"], dtype=F64), Buf(data["v"][j0:j1], offset=OFFSETS["v"], dtype=F64)
        part = Buf(count=c.n1 * width, offset=OFFSETS["out"], dtype=F64)
        work = Buf(count=wb // 8, dtype=F64)                                 # (a direct call never touches it)
        call(lib, c, X1, X2s, G, Vs, part, work, wb, n2=j1 - j0)
        check_buffers([X2s, Vs], [part, work])
        p = part.np(c.n1, width).copy()
        total = p if total is None else total + p                            # float64, slice order: what the slab kernel does
    assert np.array_equal(got.view(np.int64), total.view(np.int64)), \
        ("the split call differs from the in-order sum of its slices", c, float(np.abs(got - total).max()))
    assert ratio <= bar, (c, ratio, bar)


def test_every_family_was_reached():
    """Acceptance: all 224 instantiations ran, and the slab path at every TC of the forward and every DP of the gradient,
    for every profile, each under its derived bar.  Run the module whole: pytest -m gpu tests/test_exact_f64_gpu.py"""
    path = os.environ.get("PLX_EXACT_F64_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"|".join(map(str, fam)): {"ratio": v[0], "of_bar": v[1]} for fam, v in sorted(WORST.items())}, f, indent=1)
    if len(WORST) == 0:
        pytest.fail("no case of this module ran before the acceptance test")
    assert xf.missing_coverage(WORST) == []
    by = {}
    for (kind, profile, _, _, path_), (ratio, share) in WORST.items():
        key = (kind, profile, path_)
        by[key] = max(by.get(key, (0.0, 0.0)), (ratio, share))
    for key, (ratio, share) in sorted(by.items()):
        print(f"worst {'|'.join(key)}: {ratio:.3e} of T, {share:.3f} of its bar")
    for fam, (ratio, share) in sorted(WORST.items()):
        assert math.isfinite(ratio) and share <= 1.0, (fam, ratio, share)


# ---- the Python surface on doubles -------------------------------------------------------------------------------------
def _small(n1, n2, d, t, seed, kind="range"):
    return xf.make_data(xf.Case(f"py{seed}", "mvm", "rbf", d, t, n1, n2, kind))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("profile", xf.PROFILES)
def test_exact_matmul_on_doubles(profile):
    """square, rectangular and vector v through exact_matmul, against longdouble under the derived bar; float64 out"""
    for n1, n2, d, t, square in ((300, 300, 3, 5, True), (130, 300, 9, 1, False), (257, 65, 9, 5, False)):
        z = _small(n1, n2, d, t, seed=n1 + d)
        x2 = z["x2"]
        x1 = x2 if square else z["x1"]
        X2 = _dev(x2)
        X1 = X2 if square else _dev(x1)
        out = plx.exact_matmul(X1, X2, _dev(z["v"]), profile)
        assert out.dtype == F64 and tuple(out.shape) == (n1, t)
        want, T = xf.mvm_ld(x1, x2, z["v"], profile)
        ratio, bar = xf.entry_ratio(out.cpu().numpy(), want, T, xf.mvm_floor(n2, z["v"])), xf.bar("mvm", d, t, n2, 1)
        print(f"exact_matmul {profile} {n1}x{n2} d={d} t={t}: {ratio:.2e} (bar {bar:.2e})")
        assert ratio <= bar, (profile, n1, n2, ratio, bar)
        vec = plx.exact_matmul(X1, X2, _dev(z["v"][:, 0].copy()), profile)
        assert vec.dtype == F64 and tuple(vec.shape) == (n1,)
        assert xf.entry_ratio(vec.cpu().numpy(), want[:, 0], T[:, 0], xf.mvm_floor(n2, z["v"])) <= xf.bar("mvm", d, 1, n2, 1)


@pytest.mark.parametrize("profile", xf.PROFILES)
def test_gradcheck(profile):
    """torch.autograd.gradcheck of exact_matmul in x1, x2 and v with default tolerances, distinct points (matern12 has a
    kink at r = 0); and x1 is x2, where autograd sums the two position gradients"""
    z = _small(12, 17, 3, 2, seed=5)
    x1, x2, v = (_dev(z[k]).requires_grad_(True) for k in ("x1", "x2", "v"))
    assert torch.autograd.gradcheck(lambda a, b, w: plx.exact_matmul(a, b, w, profile), (x1, x2, v))
    x, w = _dev(z["x2"]).requires_grad_(True), _dev(z["v"]).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: plx.exact_matmul(a, a, b, profile), (x, w))


@pytest.mark.parametrize("make,profile", [(lambda: plx.RBFLattice(order=1), "rbf"),
                                          (lambda: plx.MaternLattice(nu=1.5, order=1), "matern32")])
def test_exact_twin_of_a_double_lattice_kernel(make, profile):
    try:
        n, d = 300, 3
        lat = make().double().to(DEV)
        lat.lengthscale = 0.9
        twin = plx.exact_twin(lat)
        assert twin.profile == profile and twin.lengthscale.dtype == F64 and twin.lengthscale.is_cuda
        assert torch.allclose(twin.lengthscale, lat.lengthscale, rtol=4 * 2.0 ** -52, atol=0)    # (set through the constraint)
        z = _small(n, 130, d, 5, seed=9)
        x, xs, V = _dev(z["x1"] * 3.0), _dev(z["x2"] * 3.0), _dev(np.abs(z["g"]) + 0.5)
        with torch.no_grad():
            K = twin(x, x)
            b = K @ V
            a = lat(x, x) @ V
            assert b.dtype == F64 and tuple(b.shape) == (n, 5)
            ls = float(twin.lengthscale)
            want, T = xf.mvm_ld(x.cpu().numpy() / ls, x.cpu().numpy() / ls, V.cpu().numpy(), profile)
            assert xf.entry_ratio(b.cpu().numpy(), want, T) <= xf.bar("mvm", d, 5, n, 1)
            Ks = twin(xs, x)
            W = _dev(z["v"])
            assert tuple((Ks @ V).shape) == (130, 5) and (Ks @ V).dtype == F64
            bt = Ks.t() @ W
            assert tuple(bt.shape) == (n, 5) and bt.dtype == F64
            want, T = xf.mvm_ld(x.cpu().numpy() / ls, xs.cpu().numpy() / ls, z["v"], profile)
            assert xf.entry_ratio(bt.cpu().numpy(), want, T) <= xf.bar("mvm", d, 5, 130, 1)
        e = plx.mvm_error(a, b)
        print(f"double {profile} lattice against its exact twin, n = {n}, d = {d}: {e}")
        assert all(isinstance(e[k], float) and math.isfinite(e[k]) for k in ("rel_err", "cos_err", "rel_l2"))
    finally:
        plx.lattice_cache().clear()


def test_fp32_call_unchanged_by_a_double_call_and_mixed_dtypes_refused():
    """an fp32 call after a float64 call on the same stream is bit-equal to the one before it: no shared state; a mixed
    triple is a TypeError on the device as well"""
    z = _small(257, 1500, 9, 5, seed=11)
    x1, x2, v = (_dev(z[k]) for k in ("x1", "x2", "v"))
    f1, f2, fv = x1.float(), x2.float(), v.float()
    before = plx.exact_matmul(f1, f2, fv, "matern52")
    mid = plx.exact_matmul(x1, x2, v, "matern52")
    after = plx.exact_matmul(f1, f2, fv, "matern52")
    assert before.dtype == torch.float32 and mid.dtype == F64 and _bits_equal(before.cpu(), after.cpu())
    assert float((mid - before.double()).abs().max()) > 0
    for trio in ((f1, x2, v), (x1, f2, v), (x1, x2, fv)):
        with pytest.raises(TypeError, match="one dtype"):
            plx.exact_matmul(*trio, "rbf")
    with pytest.raises(TypeError):
        plx.exact_matmul(x1.half(), x2.half(), v.half(), "rbf")
