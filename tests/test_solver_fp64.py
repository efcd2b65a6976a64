"""The native solver kernels (plx_linalg.hip, plx_cg_kernels.h, plx_pcg.hip, plx_lanczos_kernels.h) against float64, at every kernel family.

Every case calls the C ABI on fp32 data it made itself, evaluates the same expression in float64 on the CPU from the
same fp32 values (tests/solver64.py) and judges every output entry in units of the terms it sums.  The family a call
runs is a pure function of its arguments: solver64 restates the dispatch rules, every case records the families it
selects, test_every_family_was_reached (last in the module) fails if one of solver64.FAMILIES did not run.
Every buffer is allocated with exactly the size the header states, followed by a block of sentinel values: a store past
the end shows.  Inputs must come back bit-unchanged.  Masks, flags and frozen columns are exact (torch.equal).

The bars are 4x the worst ratio measured on the MI355X per quantity (DESIGN.md section 12 has the table per family).
PLX_SOLVER64_REPORT=<file> writes the worst ratios of a run as JSON."""
import ctypes
import json
import os
import zlib

import numpy as np
import pytest
import torch

from tests import solver64 as s64
from tests.gpubuf import GUARD, SENTINEL, Buf, _bits_equal, check_buffers  # noqa: F401

pytestmark = pytest.mark.gpu

# quantity -> bar = 4 x the worst measured over the module
BAR = {
    "reduction": 6.1e-7,             # column sums, |got - want| / sum |terms|: worst 1.51e-7
    "element": 4.6e-7,               # streaming updates per element, coefficient taken from the device: worst 1.15e-7
    "coefficient": 2.5e-7,           # alpha / beta against fp64 from the same fp32 scalars, relative: worst 6.1e-8
    "T": 1.4e-7,                     # plx_pcg_project per entry of T: worst 3.4e-8
    "Z": 1.2e-6,                     # plx_pcg_apply per entry of Z: worst 2.9e-7
    "lanczos_vector": 4.9e-6,        # w per entry, beta against the fp64 recurrence: worst 1.21e-6
    "lanczos_alpha_beta": 1.9e-6,    # alpha on its terms, beta^2 on the stored w: worst 4.8e-7
    "pchol_column": 1.1e-6,          # factor columns and residual diagonal per entry: worst 2.64e-7
}
WORST = {}          # (quantity, family) -> worst ratio
REACHED = set()
FLOOR = 4 * s64.FLT_MIN      # absolute error allowed where terms lie below the fp32 normal range (flushed to zero on the GPU)


@pytest.fixture(scope="module")
def lib():
    import simplex_gp_amd  # noqa: F401
    from simplex_gp_amd import _native as nv
    assert torch.cuda.is_available()
    return nv.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def record(quantity, families, ratio, what):
    families = [families] if isinstance(families, str) else list(families)
    for f in families:
        assert f in s64.FAMILIES, ("a family FAMILIES does not list", f)
        REACHED.add(f)
        WORST[(quantity, f)] = max(WORST.get((quantity, f), 0.0), ratio)
    print(f"{quantity:18s} {ratio:9.2e}  {what}  {families[0]}{' ...' if len(families) > 1 else ''}")
    assert ratio <= BAR[quantity], (quantity, ratio, BAR[quantity], what, families)


def reached(families):
    for f in [families] if isinstance(families, str) else families:
        assert f in s64.FAMILIES, f
        REACHED.add(f)


def rng(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def place_b_norm(b_norm, res, tol):
    """b_norm such that sqrt(res) / b_norm is 2 tol on even columns and tol / 2 on odd ones: no flag of a test is decided
    by rounding.  Columns with b_norm = 0 (their own case) or res <= 0 are left alone."""
    res = np.asarray(res, np.float64)
    for c in range(b_norm.numel()):
        if b_norm[c] != 0 and res[c] > 0:
            b_norm[c] = float(np.sqrt(res[c]) / (tol * (0.5 if c % 2 else 2.0)))
    return b_norm


def ok(rc, what):
    assert rc == 0, (what, rc)


# ---- coldot, cg_update, cg_step_update, cg_direction ----------------------------------------------------------------------
VDS = (1, 2, 3, 5, 7, 11, 12, 16, 17, 64, 85, 86, 128, 129, 255, 256)
SMALL_N = (0, 1, 2, 1023, 1024, 1025)


def _dot_cases():
    cases = [(n, vd) for vd in VDS for n in SMALL_N]
    cases += [(100_003, vd) for vd in (1, 2, 3, 5, 7, 11, 12, 16, 17, 64, 129, 256)]
    cases += [(1_200_003, vd) for vd in (1, 3, 12, 16)]
    return cases


def _kinds(n, vd, g, shift):
    """a, b [n][vd]: column kinds rotate through normal, all zero, one sign (no cancellation) and cancelling (the terms
    sum to 1e6 times the result)."""
    a, b = torch.randn(n, vd, generator=g), torch.randn(n, vd, generator=g)
    for c in range(vd):
        kind = (c + shift) % 4
        if kind == 1:
            a[:, c] = 0
        elif kind == 2:
            a[:, c], b[:, c] = a[:, c].abs(), b[:, c].abs()
        elif kind == 3 and n >= 2:
            u = torch.rand(n // 2, generator=g) + 0.5
            a[: n // 2 * 2, c] = torch.stack([u, -u * (1 - 2e-6)], 1).reshape(-1)
            a[n // 2 * 2:, c] = 0
            b[:, c] = 1
    return a, b


@pytest.mark.parametrize("n,vd", _dot_cases())
def test_coldot(lib, n, vd):
    """plx_coldot: every column sum against fp64 in units of sum |a b|; n = 0 and all-zero columns give exact zeros."""
    g = rng("coldot", n, vd)
    a, b = _kinds(n, vd, g, n + vd)
    A, B = Buf(a), Buf(b)
    out = Buf(count=vd)
    work = Buf(count=int(lib.plx_coldot_work_floats(vd)))
    ok(lib.plx_coldot(A.ptr, B.ptr, n, vd, out.ptr, work.ptr, stream()), "plx_coldot")
    want, T = s64.coldot64(a.numpy(), b.numpy())
    check_buffers([A, B], [out, work])
    record("reduction", s64.coldot_families("coldot_partial_kernel"), s64.entry_ratio(out.np(), want, T), f"coldot n={n} vd={vd}")


def _coef_columns(vd, g, with_pap):
    """per-column scalars with the header's special cases in rotation: normal, frozen (active = 0), rs = 0 (the
    max(rs, tiny) guard), pAp <= 0, b_norm = 0"""
    rs = torch.rand(vd, generator=g) + 0.5
    pap = torch.rand(vd, generator=g) + 0.5
    active = torch.ones(vd)
    b_norm = torch.rand(vd, generator=g) + 0.5
    for c in range(vd):
        kind = c % 6
        if kind == 1:
            active[c] = 0
        elif kind == 2:
            rs[c] = 0
        elif kind == 3 and with_pap:
            pap[c] = -0.25 if c % 12 == 3 else 0.0
        elif kind == 4:
            b_norm[c] = 0
    return rs, pap, active, b_norm


def _check_axpy(fams, name, got, y, coef_dev, x, frozen=None):
    want, T = s64.axpy64(y, coef_dev, x)
    with np.errstate(invalid="ignore"):
        record("element", fams, s64.entry_ratio(got, want, T), name)
    if frozen is not None and frozen.any():
        assert _bits_equal(torch.from_numpy(np.ascontiguousarray(got[:, frozen])), torch.from_numpy(np.ascontiguousarray(y[:, frozen]))), \
            name + ": a frozen column moved"


@pytest.mark.parametrize("n,vd", _dot_cases())
def test_cg_updates(lib, n, vd):
    """plx_cg_update, plx_cg_step_update and plx_cg_direction on the shapes of test_coldot: X, R and P per element with
    the device's own alpha (the coefficient against fp64 separately), |R|^2 from the R the kernel stored."""
    g = rng("cgu", n, vd)
    x, r, p, ap = (torch.randn(n, vd, generator=g) for _ in range(4))
    if vd > 1:
        for m in (x, r, p, ap):
            m[:, 1] = 0                                   # a column of zeros stays exactly zero
    rs, pap, active, _ = _coef_columns(vd, g, True)
    # -- plx_cg_update (alpha given)
    alpha = torch.randn(vd, generator=g)
    X, R, P, AP, AL = Buf(x), Buf(r), Buf(p), Buf(ap), Buf(alpha)
    rsn, work = Buf(count=vd), Buf(count=int(lib.plx_coldot_work_floats(vd)))
    ok(lib.plx_cg_update(X.ptr, R.ptr, P.ptr, AP.ptr, AL.ptr, n, vd, rsn.ptr, work.ptr, stream()), "plx_cg_update")
    check_buffers([P, AP, AL], [X, R, rsn, work])
    fams = s64.coldot_families("cg_update_kernel/alpha")
    _check_axpy(fams, f"cg_update X n={n} vd={vd}", X.np(n, vd), x.numpy(), alpha.numpy(), p.numpy())
    _check_axpy(fams, f"cg_update R n={n} vd={vd}", R.np(n, vd), r.numpy(), -alpha.numpy(), ap.numpy())
    want, T = s64.coldot64(R.np(n, vd), R.np(n, vd))
    record("reduction", fams, s64.entry_ratio(rsn.np(), want, T), f"cg_update |R|^2 n={n} vd={vd}")
    # -- plx_cg_step_update (alpha formed on the device)
    X, R, RS, PAP, ACT = Buf(x), Buf(r), Buf(rs), Buf(pap), Buf(active)
    rsn, al, work = Buf(count=vd), Buf(count=vd), Buf(count=int(lib.plx_coldot_work_floats(vd)))
    ok(lib.plx_cg_step_update(X.ptr, R.ptr, P.ptr, AP.ptr, RS.ptr, PAP.ptr, ACT.ptr, n, vd, rsn.ptr, al.ptr, work.ptr, stream()),
       "plx_cg_step_update")
    check_buffers([P, AP, RS, PAP, ACT], [X, R, rsn, al, work])
    fams = s64.coldot_families("cg_update_kernel/step")
    frozen = active.numpy() == 0
    a_dev = al.np()
    assert np.all(a_dev[frozen] == 0)
    record("coefficient", fams, s64.rel_ratio(a_dev, s64.alpha64(rs.numpy(), pap.numpy(), active.numpy())),
           f"cg_step_update alpha n={n} vd={vd}")
    _check_axpy(fams, f"cg_step_update X n={n} vd={vd}", X.np(n, vd), x.numpy(), a_dev, p.numpy(), frozen)
    _check_axpy(fams, f"cg_step_update R n={n} vd={vd}", R.np(n, vd), r.numpy(), -a_dev.astype(np.float64), ap.numpy(), frozen)
    with np.errstate(over="ignore", invalid="ignore"):
        Rd = R.np(n, vd).astype(np.float64)
        fin = np.isfinite(np.float32((Rd * Rd).sum(0)))       # (a pAp <= 0 column holds rs 1e30: its square leaves fp32)
    want, T = s64.coldot64(Rd[:, fin], Rd[:, fin])
    record("reduction", fams, s64.entry_ratio(rsn.np()[fin], want, T), f"cg_step_update |R|^2 n={n} vd={vd}")
    # -- plx_cg_direction
    beta = torch.randn(vd, generator=g)
    Pd, Rr, BE = Buf(p), Buf(r), Buf(beta)
    ok(lib.plx_cg_direction(Pd.ptr, Rr.ptr, BE.ptr, n, vd, stream()), "plx_cg_direction")
    check_buffers([Rr, BE], [Pd])
    _check_axpy("cg_direction_kernel", f"cg_direction n={n} vd={vd}", Pd.np(n, vd), r.numpy(), beta.numpy(), p.numpy())


# ---- plx_cg_step_direction / plx_pcg_step_direction: vector and scalar kernel ------------------------------------------------
def _direction_cases():
    cases = []
    for vd in (1, 3, 5, 7, 11, 13, 16, 255, 256):
        for n, off in ((4099, 0), (4100, 0), (4100, 1), (1, 0), (0, 0)):
            cases.append((n, vd, off))
    return cases


@pytest.mark.parametrize("which", ["cg", "pcg"])
@pytest.mark.parametrize("n,vd,off", _direction_cases())
def test_step_direction(lib, which, n, vd, off):
    """P = R + beta P (cg) / P = Z + beta P (pcg), every element, with more workgroups than columns so that the block
    residue wraps; beta, the frozen columns, the tiny guard and the activity flag as include/plx.h states them."""
    g = rng("dir", which, n, vd, off)
    p, r = torch.randn(n, vd, generator=g), torch.randn(n, vd, generator=g)
    rs, _, active, b_norm = _coef_columns(vd, g, False)
    rs_new = torch.rand(vd, generator=g) + 0.5
    rr = torch.rand(vd, generator=g) * 4 + 0.01
    tol = 1.0
    b_norm = place_b_norm(b_norm, (rs_new if which == "cg" else rr).numpy(), tol)
    P, R = Buf(p, offset=off), Buf(r)
    RSN, RS, RR, ACT, BN = Buf(rs_new), Buf(rs), Buf(rr), Buf(active), Buf(b_norm)
    beta, act_out = Buf(count=vd), Buf(count=vd)
    if which == "cg":
        ok(lib.plx_cg_step_direction(P.ptr, R.ptr, RSN.ptr, RS.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr, act_out.ptr, stream()),
           "plx_cg_step_direction")
        res = rs_new
    else:
        ok(lib.plx_pcg_step_direction(P.ptr, R.ptr, RSN.ptr, RS.ptr, RR.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr, act_out.ptr,
                                      stream()), "plx_pcg_step_direction")
        res = rr
    check_buffers([R, RSN, RS, RR, ACT, BN], [P, beta, act_out])
    fam = s64.direction_family(which, n, vd, off % 4 == 0)
    frozen = active.numpy() == 0
    b_dev = beta.np()
    assert np.all(b_dev[frozen] == 0)
    record("coefficient", fam, s64.rel_ratio(b_dev, s64.beta64(rs_new.numpy(), rs.numpy(), active.numpy())),
           f"{which}_step_direction beta n={n} vd={vd} off={off}")
    got = P.np(n, vd)
    _check_axpy(fam, f"{which}_step_direction P n={n} vd={vd} off={off}", got, r.numpy(), b_dev, p.numpy())
    if frozen.any() and n:
        assert _bits_equal(torch.from_numpy(np.ascontiguousarray(got[:, frozen])), r[:, torch.from_numpy(frozen)].contiguous()), "P != R on a frozen column"
    flag, decided = s64.active64(active.numpy(), res.numpy(), b_norm.numpy(), tol)
    assert decided.all(), "a flag of this case would be decided by rounding: move the data away from tol"
    assert torch.equal(act_out.cpu(), torch.from_numpy(flag))


@pytest.mark.parametrize("vd", (3, 12))
@pytest.mark.parametrize("n", (1, 257))
def test_cg_direction_is_the_pcg_direction(lib, n, vd):
    """plx_cg_step_direction(P, R, rs_new, rs, ...) is plx_pcg_step_direction(P, R, rs_new, rs, rr = rs_new, ...): P, beta
    and active_out agree bit for bit, P aligned and offset by one float (the vector and the scalar form each way: n vd is
    a multiple of 4 only at vd = 12), one column inactive and the others on either side of tol."""
    g = rng("cg is pcg", n, vd)
    p, r = torch.randn(n, vd, generator=g), torch.randn(n, vd, generator=g)
    rs_new, rs = (torch.rand(vd, generator=g) * 1.5 + 0.5) * n, (torch.rand(vd, generator=g) * 1.5 + 0.5) * n
    tol = 1e-3
    b_norm = (rs_new.double().sqrt() / tol * torch.where(torch.arange(vd) % 2 == 0, 0.5, 2.0)).float()
    active = torch.ones(vd)
    active[vd // 2] = 0
    for off in (0, 1):
        RSN, RS, ACT, BN = Buf(rs_new), Buf(rs), Buf(active), Buf(b_norm)
        outs = []
        for which in ("cg", "pcg"):
            P, R = Buf(p, offset=off), Buf(r)
            beta, act_out = Buf(count=vd), Buf(count=vd)
            if which == "cg":
                ok(lib.plx_cg_step_direction(P.ptr, R.ptr, RSN.ptr, RS.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr, act_out.ptr,
                                             stream()), "plx_cg_step_direction")
            else:
                ok(lib.plx_pcg_step_direction(P.ptr, R.ptr, RSN.ptr, RS.ptr, RSN.ptr, ACT.ptr, BN.ptr, tol, n, vd, beta.ptr,
                                              act_out.ptr, stream()), "plx_pcg_step_direction")
            check_buffers([R, RSN, RS, ACT, BN], [P, beta, act_out])
            reached(s64.direction_family(which, n, vd, off % 4 == 0))
            outs.append((P.cpu(), beta.cpu(), act_out.cpu()))
        for name, u, v in zip(("P", "beta", "active_out"), *outs):
            assert _bits_equal(u, v), (n, vd, off, name)
        gp, gb, gact = outs[0]
        assert not torch.equal(gp, p.reshape(-1)) and set(gact.tolist()) == {0.0, 1.0} and gb[vd // 2] == 0.0


# ---- the fused pair and the preconditioned fused direction ------------------------------------------------------------------
FUSED_TILES = (0, 1, 5, 1024, 12 * 1024 + 1, 11_719)
FUSED_N = (1, 255, 256, 257, 60_001, 1_200_003)


def _partials(rows, vd, g):
    """random positive partial sums of very different sizes (a dropped row shows)"""
    return torch.exp(torch.randn(rows, vd, generator=g) * 2) if rows else torch.zeros(0, vd)


@pytest.mark.parametrize("vd", [4, 8, 12, 16])
@pytest.mark.parametrize("j", range(6))
def test_fused_steps(lib, vd, j):
    """plx_cg_step_update_fused, plx_cg_step_direction_fused and plx_pcg_step_direction_fused: the kernels' own sums of
    the partial rows (random data of the test) against fp64, then the element updates with the device's coefficients."""
    n, ntiles = FUSED_N[(j + vd // 4) % 6], FUSED_TILES[j]
    g = rng("fused", vd, j)
    x, r, p, ap, z = (torch.randn(n, vd, generator=g) for _ in range(5))
    rs, _, active, b_norm = _coef_columns(vd, g, False)
    pp = _partials(ntiles, vd, g)
    X, R, P, AP, RS, PP, ACT = Buf(x), Buf(r), Buf(p), Buf(ap), Buf(rs), Buf(pp), Buf(active)
    al, work = Buf(count=vd), Buf(count=int(lib.plx_cg_fused_work_floats(vd)))
    ok(lib.plx_cg_step_update_fused(X.ptr, R.ptr, P.ptr, AP.ptr, RS.ptr, PP.ptr, ntiles, ACT.ptr, n, vd, al.ptr, work.ptr, stream()),
       "plx_cg_step_update_fused")
    check_buffers([P, AP, RS, PP, ACT], [X, R, al, work])
    fam = s64.fused_family("cg_step_update_fused_kernel", vd)
    frozen = active.numpy() == 0
    pap64, _ = s64.colsum64(pp.numpy().reshape(ntiles, vd))
    a_dev = al.np()
    assert np.all(a_dev[frozen] == 0)
    # alpha = rs / max(sum of the partials, tiny): the partials are positive, so the relative error of alpha is that of the sum
    record("reduction", fam, s64.rel_ratio(a_dev, s64.alpha64(rs.numpy(), pap64, active.numpy())), f"update_fused alpha n={n} tiles={ntiles} vd={vd}")
    _check_axpy(fam, f"update_fused X n={n} vd={vd}", X.np(n, vd), x.numpy(), a_dev, p.numpy(), frozen)
    _check_axpy(fam, f"update_fused R n={n} vd={vd}", R.np(n, vd), r.numpy(), -a_dev.astype(np.float64), ap.numpy(), frozen)
    Rd = R.np(n, vd).astype(np.float64)
    with np.errstate(over="ignore"):
        fin = np.isfinite(np.float32((Rd * Rd).sum(0)))
    want, T = s64.coldot64(Rd[:, fin], Rd[:, fin])
    got = s64.colsum64(work.np(s64.FUSED_BLOCKS, vd))[0]
    record("reduction", fam, s64.entry_ratio(got[fin], want, T), f"update_fused |R|^2 partials n={n} vd={vd}")

    # direction_fused: its own sum of 256 partial rows (mixed signs: judged on the terms), beta, flag, P = R + beta P
    part = torch.randn(s64.FUSED_BLOCKS, vd, generator=g) * torch.exp(torch.randn(s64.FUSED_BLOCKS, vd, generator=g))
    part[:, 0] = part[:, 0].abs()
    part[:, 3] = 0
    W, Pd, Rr = Buf(part), Buf(p), Buf(r)
    rsn, beta, act_out = Buf(count=vd), Buf(count=vd), Buf(count=vd)
    tol = 1e-3
    b_norm = place_b_norm(b_norm, s64.colsum64(part.numpy())[0], tol)
    BN = Buf(b_norm)
    ok(lib.plx_cg_step_direction_fused(Pd.ptr, Rr.ptr, W.ptr, RS.ptr, ACT.ptr, BN.ptr, tol, n, vd, rsn.ptr, beta.ptr,
                                       act_out.ptr, stream()), "plx_cg_step_direction_fused")
    check_buffers([Rr, W, RS, ACT], [Pd, rsn, beta, act_out])
    fam = s64.fused_family("cg_step_direction_fused_kernel", vd)
    want, T = s64.colsum64(part.numpy())
    rsn_dev = rsn.np()
    record("reduction", fam, s64.entry_ratio(rsn_dev, want, T), f"direction_fused rs_new n={n} vd={vd}")
    b_dev = beta.np()
    assert np.all(b_dev[frozen] == 0)
    record("coefficient", fam, s64.rel_ratio(b_dev, s64.beta64(rsn_dev, rs.numpy(), active.numpy())),
           f"direction_fused beta n={n} vd={vd}")
    _check_axpy(fam, f"direction_fused P n={n} vd={vd}", Pd.np(n, vd), r.numpy(), b_dev, p.numpy())
    with np.errstate(invalid="ignore"):
        flag, decided = s64.active64(active.numpy(), np.maximum(want, 0), b_norm.numpy(), tol)
        neg = want < 0                                       # sqrt of a negative sum: NaN > tol is false
    flag[neg] = 0
    assert (decided | neg).all()
    assert torch.equal(act_out.cpu(), torch.from_numpy(flag))

    # pcg_step_direction_fused: <R, Z> from nrz partial rows, |R|^2 from 256
    nrz = ntiles
    rzp, rrp = _partials(nrz, vd, g), _partials(s64.FUSED_BLOCKS, vd, g) * 1e-2
    RZP, RRP, Pd, Zz = Buf(rzp), Buf(rrp), Buf(p), Buf(z)
    rzn, rro, beta, act_out = Buf(count=vd), Buf(count=vd), Buf(count=vd), Buf(count=vd)
    tol = 1.0
    b_norm = place_b_norm(b_norm, s64.colsum64(rrp.numpy())[0], tol)
    BN = Buf(b_norm)
    ok(lib.plx_pcg_step_direction_fused(Pd.ptr, Zz.ptr, RZP.ptr, nrz, RRP.ptr, RS.ptr, ACT.ptr, BN.ptr, tol, n, vd, rzn.ptr,
                                        rro.ptr, beta.ptr, act_out.ptr, stream()), "plx_pcg_step_direction_fused")
    check_buffers([Zz, RZP, RRP, RS, ACT], [Pd, rzn, rro, beta, act_out])
    fam = s64.fused_family("pcg_step_direction_fused_kernel", vd)
    want, T = s64.colsum64(rzp.numpy().reshape(nrz, vd))
    record("reduction", fam, s64.entry_ratio(rzn.np(), want, T), f"pcg_direction_fused rz_new n={n} nrz={nrz} vd={vd}")
    want_rr, T = s64.colsum64(rrp.numpy())
    record("reduction", fam, s64.entry_ratio(rro.np(), want_rr, T), f"pcg_direction_fused rr n={n} vd={vd}")
    b_dev = beta.np()
    assert np.all(b_dev[frozen] == 0)
    record("coefficient", fam, s64.rel_ratio(b_dev, s64.beta64(rzn.np(), rs.numpy(), active.numpy())),
           f"pcg_direction_fused beta n={n} vd={vd}")
    _check_axpy(fam, f"pcg_direction_fused P n={n} vd={vd}", Pd.np(n, vd), z.numpy(), b_dev, p.numpy())
    flag, decided = s64.active64(active.numpy(), want_rr, b_norm.numpy(), tol)
    assert decided.all()
    assert torch.equal(act_out.cpu(), torch.from_numpy(flag))


def test_fused_steps_refuse_what_they_cannot_serve(lib):
    """vd = 11 and a buffer 4 bytes past a 16-byte boundary are errors and leave every output untouched."""
    n = 300
    g = rng("refuse")
    for vd, off in ((11, 0), (12, 1)):
        mk = lambda o=0: Buf(torch.randn(n, vd, generator=g), offset=o)      # noqa: E731
        X, R, P, AP, Z = mk(), mk(), mk(off), mk(), mk()
        small = [Buf(torch.rand(vd, generator=g) + 0.5) for _ in range(4)]
        PP = Buf(torch.rand(5 * vd, generator=g), offset=off)
        outs = [Buf(count=vd) for _ in range(5)]
        work = Buf(count=256 * 16)
        assert lib.plx_cg_step_update_fused(X.ptr, R.ptr, P.ptr, AP.ptr, small[0].ptr, PP.ptr, 5, small[1].ptr, n, vd, outs[0].ptr,
                                            work.ptr, stream()) != 0
        assert lib.plx_cg_step_direction_fused(P.ptr, R.ptr, work.ptr, small[0].ptr, small[1].ptr, small[2].ptr, 1.0, n, vd,
                                               outs[1].ptr, outs[2].ptr, outs[3].ptr, stream()) != 0
        assert lib.plx_pcg_step_direction_fused(P.ptr, Z.ptr, PP.ptr, 5, work.ptr, small[0].ptr, small[1].ptr, small[2].ptr, 1.0, n,
                                                vd, outs[1].ptr, outs[4].ptr, outs[2].ptr, outs[3].ptr, stream()) != 0
        torch.cuda.synchronize()
        for b in [X, R, P, AP, Z, PP, work] + small + outs:
            assert b.unchanged() and b.guards_intact()
    assert lib.plx_cg_fused_work_floats(11) < 0


# ---- plx_pcg_factor_to_half, plx_pcg_project, plx_pcg_apply ------------------------------------------------------------------------
def test_factor_to_half(lib):
    """bit-equal to torch.Tensor.half() (round to nearest even) on ties, the largest finite half and the first value that
    rounds past it (-> inf, as IEEE conversion does: the caller must keep the factor inside the range), half subnormals,
    values below them, both zeros, and random data."""
    table = [1.0, 1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, 1.0 + 2 ** -11 + 2 ** -20, 1.0 + 2 ** -10, 2049.0, 2051.0, 65504.0, 65519.0,
             65519.996, 65520.0, 1e5, 3e38, 2 ** -14, 2 ** -14 - 2 ** -25, 2 ** -24, 2 ** -25, 2 ** -25 * 1.0001, 3 * 2 ** -25, 2 ** -26,
             1e-30, 1e-45, 0.0, 6.1e-5, 5.96e-8, 0.333333343]
    v = torch.tensor(table + [-x for x in table], dtype=torch.float32)
    kp, ld = 16, 128
    src = torch.randn(kp, ld, generator=rng("half")) * torch.exp(torch.randn(kp, ld, generator=rng("half2")) * 4)
    src.reshape(-1)[: v.numel()] = v
    S, D = Buf(src), Buf(count=kp * ld, dtype=torch.float16)
    ok(lib.plx_pcg_factor_to_half(S.ptr, ld, kp, D.ptr, stream()), "plx_pcg_factor_to_half")
    check_buffers([S], [D])
    assert _bits_equal(D.cpu(), src.reshape(-1).half())
    assert torch.isinf(D.cpu()[table.index(65520.0)]) and D.cpu()[table.index(65519.996)] == 65504.0
    reached("pcg_to_half_kernel")


def _factor(kind, kp, k, n, ld, g, half):
    """L^T [kp][ld]: rows k.., columns n.. zero (include/plx.h)."""
    Lt = torch.zeros(kp, ld)
    if kind == "random":
        Lt[:k, :n] = torch.randn(k, n, generator=g) * 0.3
    elif kind == "one_tile":              # a single 64-row tile is not zero: a dropped tile shows
        t0 = (n // 64) // 2 * 64
        Lt[:k, t0: min(t0 + 64, n)] = torch.randn(k, min(t0 + 64, n) - t0, generator=g)
    elif kind == "integers":              # small integers: L^T R is exact in fp32 whatever the order of the sums
        Lt[:k, :n] = torch.randint(-3, 4, (k, n), generator=g).float()
    if half:
        Lt = Lt.half().float()
    return Lt


def _cinv(Lt, k, kp, n, noise):
    L = Lt[:k, :n].double().numpy()
    cinv = np.eye(kp) / noise
    cinv[:k, :k] = np.linalg.inv(L @ L.T + noise * np.eye(k))
    cinv = (cinv + cinv.T) / 2
    return cinv


def _device_factor(lib, Lt, half):
    kp, ld = Lt.shape
    F = Buf(Lt)
    if not half:
        return F, 0
    H = Buf(count=kp * ld, dtype=torch.float16)
    ok(lib.plx_pcg_factor_to_half(F.ptr, ld, kp, H.ptr, stream()), "to_half")
    assert _bits_equal(H.cpu(), Lt.reshape(-1).half())
    H.before = H.view.cpu().clone()
    reached("pcg_to_half_kernel")
    return H, 1


KPS = (16, 32, 48, 64, 80, 96, 112, 128, 144, 256, 400, 1008, 1024)
PROJECT_N = (1, 63, 64, 65, 4097, 700)


def _project_cases():
    cases = []
    for half in (False, True):
        for j, kp in enumerate(KPS):
            n = PROJECT_N[(j + half) % 6]
            t = (j * 5 + 7 * half) % 16 + 1
            kind = ("random", "one_tile", "integers")[(j + half) % 3]
            cases.append((half, kp, n, t, kind if n > 64 or kind != "one_tile" else "random"))
        cases.append((half, 16, 1_100_000, 16 if half else 13, "random"))
        cases.append((half, 48, 4097, 11 - half, "one_tile"))
        cases.append((half, 144, 65, 16, "integers"))
    return cases


@pytest.mark.parametrize("half,kp,n,t,kind", _project_cases())
def test_pcg_project(lib, half, kp, n, t, kind):
    """T = Cinv (L^T R) per entry against |Cinv| (|L|^T |R|); the padding rows k..kp are exactly 0 (zero rows of the
    factor, Cinv = identity / sigma^2 there).  With small-integer L and R the gram sums are exact, and T must agree with
    the fp64 product to the rounding of its own store."""
    g = rng("project", half, kp, n, t)
    ld = (n + 63) // 64 * 64
    k = kp if kp in (16, 128, 1024) else kp - 3
    Lt = _factor(kind, kp, k, n, ld, g, half)
    R = torch.randint(-4, 5, (n, t), generator=g).float() if kind == "integers" else torch.randn(n, t, generator=g)
    noise = 0.37
    cinv = _cinv(Lt, k, kp, n, noise)
    F, ftype = _device_factor(lib, Lt, half)
    Rb, Cb = Buf(R), Buf(cinv, dtype=torch.float64)
    Tb = Buf(count=kp * 16, fill=SENTINEL)
    work = Buf(count=int(lib.plx_pcg_work_floats(n, kp, t)))
    ok(lib.plx_pcg_project(F.ptr, ftype, ld, kp, Rb.ptr, n, t, Cb.ptr, Tb.ptr, work.ptr, stream()), "plx_pcg_project")
    check_buffers([F, Rb, Cb], [Tb, work])
    Tdev = Tb.np(kp, 16)
    want, T = s64.project64(Lt[:, :n].numpy(), R.numpy(), cinv)
    assert np.all(Tdev[k:, :t] == 0)
    fams = s64.project_families(kp, half)
    record("T", fams, s64.entry_ratio(Tdev[:, :t], want, T), f"project {kind} kp={kp} n={n} t={t} {s64.HALF[half]}")
    if kind == "integers":
        assert np.all(np.abs(Tdev[:, :t] - want) <= 2.0 ** -23 * np.abs(want) + 1e-13 * T), "exact gram sums: T may only differ by its own rounding"


APPLY_N = (4097, 4160, 777, 1, 64, 65)


def _apply_cases():
    cases = []
    for half in (False, True):
        for t in range(1, 17):
            kp = (16, 32, 144)[t % 3]
            k = (0, 1, kp - 1, kp)[(t + half) % 4]
            cases.append((half, t, kp, k, APPLY_N[(t + 3 * half) % 6], (t + half) % 2 == 0))
    return cases


def _run_apply(lib, half, t, kp, k, n, with_rz, g):
    ld = (n + 63) // 64 * 64
    Lt = _factor("random", kp, kp, n, ld, g, half)           # rows k..kp are NOT zero here: only k rows may be used
    R = torch.randn(n, t, generator=g)
    Tm = torch.randn(kp, 16, generator=g)
    scale = torch.tensor([0.75, 1.0 / 0.37])
    F, ftype = _device_factor(lib, Lt, half)
    Rb, Tb, Sb = Buf(R), Buf(Tm), Buf(scale)
    Z, rz = Buf(count=n * t), Buf(count=t)
    work = Buf(count=int(lib.plx_pcg_work_floats(n, kp, t)))
    ok(lib.plx_pcg_apply(F.ptr, ftype, ld, kp, k, Rb.ptr, n, t, Tb.ptr, Sb.ptr, Z.ptr, rz.ptr if with_rz else None, work.ptr, stream()),
       "plx_pcg_apply")
    check_buffers([F, Rb, Tb, Sb], [Z, rz, work])
    what = f"apply kp={kp} k={k} n={n} t={t} {s64.HALF[half]} rz={'given' if with_rz else 'NULL'}"
    fams = s64.apply_families(n, t, half, with_rz)
    Zd = Z.np(n, t)
    want, T = s64.apply64(Lt[:, :n].numpy(), k, R.numpy(), Tm.numpy(), scale.numpy())
    record("Z", fams[0], s64.entry_ratio(Zd, want, T), what)
    want, T = s64.coldot64(R.numpy(), Zd)
    if with_rz:
        got = rz.np()
    else:
        assert rz.unchanged()
        off, rows = int(lib.plx_pcg_rz_partial_offset(kp)), int(lib.plx_pcg_rz_partial_rows(n, ftype))
        assert rows == s64.rz_rows(n, half)
        got = work.np()[off: off + rows * t].reshape(rows, t).astype(np.float64).sum(0)
    record("reduction", fams, s64.entry_ratio(got, want, T), what + " <R, Z>")


@pytest.mark.parametrize("half,t,kp,k,n,with_rz", _apply_cases())
def test_pcg_apply(lib, half, t, kp, k, n, with_rz):
    """Z = (s0 R - L T) s1 per entry against (|s0 R| + |L| |T|) |s1| for every column count and both factor types, k = 0,
    1, kp - 1 and kp, n odd and even, n = ld - 63 and n = ld; <R, Z> from d_rz or from the partial rows left in d_work."""
    _run_apply(lib, half, t, kp, k, n, with_rz, rng("apply", half, t))


@pytest.mark.parametrize("half", [False, True])
def test_pcg_apply_large(lib, half):
    """n above 1,048,576 at kp = 16: with the fp32 factor <R, Z> has 4297 partial rows and coldot_final_kernel's four-way
    unrolled loop runs."""
    _run_apply(lib, half, 5 if half else 3, 16, 16, 1_100_000 + half, True, rng("applyL", half))


def test_pcg_apply_refuses_misaligned_rows(lib):
    n, kp, t = 300, 16, 4
    g = rng("applyR")
    F = Buf(torch.zeros(kp, 320))
    Tb, Sb = Buf(torch.randn(kp, 16, generator=g)), Buf(torch.ones(2))
    for roff, zoff in ((1, 0), (0, 1)):
        work = Buf(count=int(lib.plx_pcg_work_floats(n, kp, t)))
        R, Z, rz = Buf(torch.randn(n, t, generator=g), offset=roff), Buf(count=n * t, offset=zoff), Buf(count=t)
        assert lib.plx_pcg_apply(F.ptr, 0, 320, kp, kp, R.ptr, n, t, Tb.ptr, Sb.ptr, Z.ptr, rz.ptr, work.ptr, stream()) != 0
        torch.cuda.synchronize()
        assert Z.unchanged() and rz.unchanged() and work.unchanged()
        # three columns need no alignment
        R3, Z3 = Buf(torch.randn(n, 3, generator=g), offset=roff), Buf(count=n * 3, offset=zoff)
        ok(lib.plx_pcg_apply(F.ptr, 0, 320, kp, kp, R3.ptr, n, 3, Tb.ptr, Sb.ptr, Z3.ptr, rz.ptr, work.ptr, stream()), "apply t = 3")
        assert _bits_equal(Z3.cpu(), R3.before) and Z3.guards_intact()            # L = 0, scales 1: Z = R
        reached(s64.apply_families(n, 3, False, True))


# ---- batched pivoted Cholesky without a lattice ------------------------------------------------------------------------------------
def _spd(n, coupling, seed):
    """dense SPD test matrix in fp64, rounded to fp32: RBF on random 2-d points plus a jitter, scaled so that the
    diagonal is a geometric ladder (consecutive pivots stay well apart)."""
    g = np.random.default_rng(seed)
    x = g.uniform(0, 1, (n, 2)) * np.sqrt(n)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    K = np.exp(-d2 / coupling ** 2)
    step = max(1.0025, 1 + 10.0 / n)
    s = step ** (-g.permutation(n) / 2.0)
    A = K * np.outer(s, s) + 1e-2 * np.diag(s * s)
    return A.astype(np.float32)


_SPD = {}


def _spd_state(n, coupling, m_done):
    """(A32, L_done fp32 [m_done][n], diag fp32): the state after m_done sequential fp64 steps, rounded to fp32"""
    key = (n, coupling)
    if key not in _SPD:
        A = _spd(n, coupling, 1000 + n)
        _SPD[key] = (A, {})
    A, states = _SPD[key]
    if m_done not in states:
        piv, cols, _, d, gaps = s64.pchol64(A, np.diag(A), [], m_done, 0.0)
        states[m_done] = (cols.astype(np.float32), d.astype(np.float32))
    return (A,) + states[m_done]


def _run_batch(lib, A, L_done, diag, kp, m_done, nb, t, rank, tol_abs, exact):
    """select + factor_batch as solvers.LatticePreconditioner calls them; d_rows = A[:, cand]"""
    n = A.shape[0]
    ld = (n + 63) // 64 * 64
    Lt = torch.full((kp, ld), SENTINEL)
    Lt[:, n:] = 0
    Lt[:m_done, :n] = torch.from_numpy(L_done)
    LT, D = Buf(Lt), Buf(diag)
    RK = Buf(rank, dtype=torch.int32) if rank is not None else None
    cand, acc = Buf(count=16, dtype=torch.int32), Buf(count=2, dtype=torch.int32)
    work = Buf(count=int(lib.plx_pchol_work_bytes(ld, kp)), dtype=torch.uint8)
    rkp = RK.ptr if RK is not None else None
    ok(lib.plx_pchol_select(D.ptr, rkp, n, nb, ld, kp, cand.ptr, work.ptr, stream()), "plx_pchol_select")
    c = cand.cpu()[:nb].tolist()
    assert c == s64.top_candidates(diag, nb, rank), "plx_pchol_select: not the nb largest entries in order"
    assert D.unchanged() and cand.guards_intact()
    rhs = Buf(count=n * t, fill=SENTINEL)
    ok(lib.plx_pchol_onehot(cand.ptr, nb, n, t, rhs.ptr, stream()), "plx_pchol_onehot")
    E = torch.zeros(n, t)
    E[c, list(range(nb))] = 1
    assert torch.equal(rhs.cpu(n, t), E) and rhs.guards_intact()
    rows = torch.zeros(n, t)
    rows[:, :nb] = torch.from_numpy(A[:, c])
    RW, SC = Buf(rows), Buf(torch.tensor([1.0, 1.0]))
    ok(lib.plx_pchol_factor_batch(LT.ptr, ld, kp, m_done, RW.ptr, t, SC.ptr, cand.ptr, nb, D.ptr, rkp, n, tol_abs, exact, acc.ptr,
                                  work.ptr, stream()), "plx_pchol_factor_batch")
    check_buffers([RW, SC] + ([RK] if RK else []), [LT, D, cand, acc, work])
    assert cand.cpu()[:nb].tolist() == c
    a, planned = acc.cpu().tolist()
    return c, a, planned, LT.cpu(kp, ld), D.cpu()


PCHOL_N = (50, 1023, 1025, 4000)


def _pchol_cases():
    cases = []
    for a, nb in enumerate((1, 2, 7, 16)):
        for b, m in enumerate((0, 1, 16, 17, "last")):
            n = PCHOL_N[(a + b) % 4]
            kp = 48 if n > 50 else 32
            cases.append((n, kp, kp - nb if m == "last" else m, nb, 0.7 if (a + b) % 3 else 1.7))
    # strongly coupled: the plan ends before the batch does and pchol_step_kernel writes the columns after it
    cases += [(1023, 48, 0, 16, 8.0), (1023, 48, 3, 16, 8.0)]
    return cases


@pytest.mark.parametrize("n,kp,m_done,nb,coupling", _pchol_cases())
def test_pchol_batch(lib, n, kp, m_done, nb, coupling):
    """One batch of plx_pchol_select / onehot / factor_batch from the state the sequential fp64 algorithm leaves after
    m_done steps (rounded to fp32), on a dense SPD matrix: the same pivots in the same order (the reference's pivots are
    at least 1e-3 apart, asserted), every accepted column per entry against (|row| + sum |L| |L|) / sqrt(pivot), the
    residual diagonal, and with exact_steps the batch ends exactly where the argmax leaves the candidates."""
    A, L_done, diag = _spd_state(n, coupling, m_done)
    t = nb if nb == 1 else min(16, nb + (m_done + n) % 3)
    cand, a, planned, Lt, dnew = _run_batch(lib, A, L_done, diag, kp, m_done, nb, t, None, 0.0, 1)
    piv, cols, terms, d64, gaps = s64.pchol64(A, diag, L_done, nb, 0.0, allowed=set(cand))
    assert len(piv) >= 1 and min(gaps) >= 1e-3, ("the test matrix does not keep its pivots apart", gaps)
    assert 1 <= planned <= a and a == len(piv), (a, planned, len(piv))
    if coupling == 8.0:
        assert a > planned, "this case exists to run the steps behind the plan"
    # (the step kernel counts as reached where it wrote a column: a pivot accepted after the planned ones)
    fams = s64.pchol_batch_families(m_done, t, nb, a > planned) + ["pchol_onehot_kernel"]
    assert _bits_equal(Lt[:m_done, :n], torch.from_numpy(L_done)), "finished columns were written"
    assert torch.all(Lt[:, n:] == 0) and torch.all(Lt[m_done + a:, :n] == SENTINEL), "a row the batch does not own was written"
    got = Lt[m_done: m_done + a, :n].numpy()
    for j, p in enumerate(piv):
        assert dnew[p] == 0, "the residual diagonal at a pivot is exactly 0"
    # every column from the fp32 columns before it as the kernel stored them (the inputs of its own step); the fp64 chain
    # decides the pivots and judges the residual diagonal.  (Far entries of an RBF matrix lie below the fp32 normal range: FLOOR)
    cols_given, terms_given = s64.pchol_columns_given(A, diag, L_done, got, piv, 0.0)
    record("pchol_column", fams, s64.entry_ratio(got, cols_given, terms_given, FLOOR), f"pchol n={n} m_done={m_done} nb={nb} t={t} accepted={a} planned={planned}")
    # the residual diagonal: d - sum col^2, each step in units of d + col^2
    Td = diag.astype(np.float64) + (cols ** 2).sum(0)
    record("pchol_column", fams, s64.entry_ratio(dnew.numpy(), d64, Td, FLOOR), f"pchol diag n={n} m_done={m_done} nb={nb}")


@pytest.mark.parametrize("t", range(1, 17))
def test_pchol_panel_widths(lib, t):
    """the transposed panel apply at every column count t = 1..16 (nb = 1 pivot, m_done = 5 finished columns)"""
    A, L_done, diag = _spd_state(1023, 0.7, 5)
    cand, a, planned, Lt, dnew = _run_batch(lib, A, L_done, diag, 16, 5, 1, t, None, 0.0, 0)
    piv, cols, terms, d64, gaps = s64.pchol64(A, diag, L_done, 1, 0.0)
    assert a == 1 and cand == piv and gaps[0] >= 1e-3
    record("pchol_column", s64.pchol_batch_families(5, t, 1, 0), s64.entry_ratio(Lt[5:6, :1023].numpy(), cols, terms, FLOOR), f"pchol panel t={t}")


@pytest.mark.parametrize("use_rank", [False, True])
def test_pchol_exact_ties_and_tol(lib, use_rank):
    """A diagonal matrix with repeated entries: every tie is exact, the order is decided by d_rank (lower first) or, with
    NULL, by the lower index; entries at or below tol_abs give zero columns that still count as accepted."""
    n, kp, nb = 300, 16, 16
    g = np.random.default_rng(5)
    v = np.float32(1.0 + 0.25 * (np.arange(n) // 3 % 5))
    v[g.permutation(n)[:290]] *= np.float32(2.0 ** -30)          # 10 entries stay large, the rest lie below tol_abs = 1e-6
    v[7] = 0
    rank = g.permutation(n) if use_rank else None
    A = np.diag(v)
    cand, a, planned, Lt, dnew = _run_batch(lib, A, np.zeros((0, n), np.float32), v, kp, 0, nb, nb, rank, 1e-6, 1)
    piv, cols, terms, d64, gaps = s64.pchol64(A, v, [], nb, 1e-6, rank=rank)
    assert a == nb == len(piv)
    assert torch.equal(torch.tensor(cand), torch.tensor(s64.top_candidates(v, nb, rank)))
    got_piv = []
    for j in range(nb):
        nz = torch.nonzero(Lt[j, :n]).reshape(-1).tolist()
        got_piv.append(nz[0] if len(nz) == 1 else -1)
    big = [p for p in piv if v[p] > 1e-6]
    assert len(big) == 10 and torch.equal(torch.tensor(got_piv[:10]), torch.tensor(piv[:10])), (got_piv, piv)
    assert torch.equal(Lt[:nb, :n] != 0, torch.from_numpy(cols != 0)), "one entry per column at its pivot, zero columns below tol_abs"
    assert torch.all(Lt[10:nb] == 0) and torch.equal(dnew, torch.from_numpy(d64.astype(np.float32)))
    record("pchol_column", s64.pchol_batch_families(0, nb, nb, 0) + ["pchol_onehot_kernel"], s64.entry_ratio(Lt[:nb, :n].numpy(), cols, terms),
           f"pchol ties rank={'given' if use_rank else 'NULL'}")


# ---- plx_lanczos_step, single steps ------------------------------------------------------------------------------------------------
def _lanczos_cases():
    cases = []
    for n in (1, 255, 257):
        cases += [(n, i) for i in (0, 1, 2, 63, 64, 254, 255)]
    cases += [(65_536, i) for i in (0, 63, 255)] + [(65_537, i) for i in (1, 2, 64, 254)]
    cases += [(262_144, 0), (262_144, 64), (262_145, 3), (262_145, 0)]
    cases += [(n, i) for n in (1_048_576, 1_048_577, 2_097_152) for i in (0, 3)]
    # the span edges above all give 1, 2, 65, 129 or 256 workgroups: 0, 1 or 2 modulo 8.  lz_sum_groups walks the groups
    # in four slices, two loads per trip, so its tail depends on the count modulo 8: counts 6, 7, 12, 69, 76 and 135
    cases += [(1283, 2), (1792, 1), (3000, 5), (70_000, 3), (310_000, 3), (1_100_000, 3)]
    return cases


@pytest.mark.parametrize("n,i", _lanczos_cases())
@pytest.mark.parametrize("near_span", [False, True])
def test_lanczos_step(lib, n, i, near_span):
    """One step from a given basis: w and the next basis vector per entry against |w| + sum_j |c_j| |q_j|, alpha against
    the terms of q_i . w, beta against the norm of the w the kernel stored (and against the fp64 recurrence in units of
    the terms).  Q is orthonormal in fp64 then rounded; near_span: w lies almost in span(Q), so beta is small against |w|.
    The padding columns n..ld hold NaN: nothing may become NaN, the padding stays, a repeated step is bit-identical."""
    g = np.random.default_rng([n, i, int(near_span)])
    rows = i + 1
    ld = (n + 3) // 4 * 4 + (4096 if (n + i) % 2 else 0)
    M = g.standard_normal((n, rows))
    if n >= rows:
        M, _ = np.linalg.qr(M)
    else:
        M /= np.linalg.norm(M, axis=0, keepdims=True)
    Q = np.ascontiguousarray(M.T).astype(np.float32)
    del M
    w = g.standard_normal(n)
    if near_span:
        w = Q.astype(np.float64).T @ g.standard_normal(rows) * 3 + 1e-3 * w
    w = w.astype(np.float32)
    basis = torch.full((rows + 1, ld), float("nan"))
    basis[:rows, :n] = torch.from_numpy(Q)
    nwork = int(lib.plx_lanczos_work_floats(n))
    assert nwork > 0
    outs = []
    for rep in range(2):
        QB, W = Buf(basis), Buf(w)
        alphas, betas, work = Buf(count=256), Buf(count=256), Buf(count=nwork)
        ok(lib.plx_lanczos_step(QB.ptr, ld, W.ptr, n, i, alphas.ptr, betas.ptr, work.ptr, stream()), "plx_lanczos_step")
        check_buffers([], [QB, W, alphas, betas, work])
        outs.append((QB.cpu(rows + 1, ld), W.cpu(), alphas.cpu(), betas.cpu()))
        del QB, W
    assert all(_bits_equal(x, y) for x, y in zip(outs[0], outs[1])), "a repeated step differs"
    qb, wd, al, be = outs[0]
    assert _bits_equal(qb[:rows], basis[:rows]) and _bits_equal(qb[rows, n:], basis[rows, n:]), "the basis or its padding was written"
    keep = torch.ones(256, dtype=torch.bool)
    keep[i] = False
    assert torch.all(al[keep] == SENTINEL) and torch.all(be[keep] == SENTINEL)
    ref = s64.lanczos_step64(Q, w, i)
    fams = s64.lanczos_families(n)
    what = f"lanczos n={n} i={i} ld={ld}{' near span' if near_span else ''}"
    record("lanczos_vector", fams, s64.entry_ratio(wd.numpy(), ref["w"], ref["Tw"]), what + " w")
    a_dev, b_dev = float(al[i]), float(be[i])
    record("lanczos_alpha_beta", fams, s64.entry_ratio(a_dev, ref["alpha"], ref["Talpha"]), what + " alpha")
    wd64 = wd.numpy().astype(np.float64)
    record("lanczos_alpha_beta", fams, s64.entry_ratio(b_dev * b_dev, wd64 @ wd64, wd64 @ wd64), what + " beta^2 from the stored w")
    record("lanczos_vector", fams, s64.entry_ratio(b_dev, ref["beta"], np.linalg.norm(ref["Tw"])), what + " beta")
    qn = qb[rows, :n].numpy()
    record("element", fams, s64.entry_ratio(qn, wd64 / max(b_dev, 1e-30), np.abs(wd64) / max(b_dev, 1e-30)), what + " next vector")


def test_lanczos_refuses_more_than_it_serves(lib):
    assert lib.plx_lanczos_work_floats(2_097_153) < 0 and lib.plx_lanczos_work_floats(2_097_152) > 0
    small = Buf(count=1024)
    assert lib.plx_lanczos_step(small.ptr, 2_097_156, small.ptr, 2_097_153, 0, small.ptr, small.ptr, small.ptr, stream()) != 0
    assert lib.plx_lanczos_step(small.ptr, 64, small.ptr, 60, 256, small.ptr, small.ptr, small.ptr, stream()) != 0
    torch.cuda.synchronize()
    assert small.unchanged()


# ---- acceptance ------------------------------------------------------------------------------------------------------------------
def test_every_family_was_reached():
    """Acceptance: every family of solver64.FAMILIES ran in this module, except those listed as unreachable (at most 3).
    Run the module whole: pytest -m gpu tests/test_solver_fp64.py"""
    path = os.environ.get("PLX_SOLVER64_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({f"{q}|{fam}": v for (q, fam), v in sorted(WORST.items())}, f, indent=1)
    if len(REACHED) == 0:
        pytest.fail("no case of this module ran before the acceptance test")
    assert len(s64.UNREACHABLE) <= 3
    missing = [f for f in s64.FAMILIES if f not in REACHED and f not in s64.UNREACHABLE]
    assert not missing, missing
    for (q, fam), v in sorted(WORST.items()):
        assert v <= BAR[q], (q, fam, v)
