"""The fused position gradient (plx_apply_backward) against float64 at every shape family it accepts.

plx_apply_backward accepts 60 (d, MAXCH) families -- MAXCH = 1 up to 64 float4 chunks per vertex row, 2 above -- run by
slice_contract_d_kernel<d + 1, MAXCH> for d <= 20 and by the run-time slice_contract_kernel<MAXCH> for d >= 21 (and for
every d when the "contract_v" tune is 0).  Each family runs at the smallest and the largest L of its band, on Gaussian
clouds, on one simplex (long vertex rows) and on isolated points (a vanishing true gradient), and is compared with the
float64 operator of tests/lattice64.py built on the same duplicate-free structure.

Bars, in float64.  grad_x is a difference of products: ||got - want|| <= TAU ||T|| with T the size of those products
(lattice64.contract64), and, where the gradient does not vanish (||want|| >= 0.1 ||T||), rel-L2 <= REL_X as well.  grad_src
and the forward product of the stacked matrix: rel-L2 <= REL.  The worst ratio of every family is printed at the end of the
module (pytest -s).
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from tests.lattice64 import CLOUDS, Lattice64, cloud, contract64, grad_x_ratios, rel_l2, stack64

pytestmark = pytest.mark.gpu

# Starting bars 1e-5 of ||T||, rel 2e-5 and rel 1e-5, tightened to 4x the measured worst over all 60 families
# (table in DESIGN.md section 10): 1.8e-7 of ||T||, rel 4.9e-7 and rel 8.8e-7.
TAU = 7e-7        # grad_x error / size of its terms
REL_X = 2e-6      # grad_x rel-L2 where the gradient does not vanish
REL = 3.5e-6      # grad_src and forward rel-L2
N = 701           # odd: the last workgroup of every launch is partial
PLX_ERR_INVALID = 1                                           # plx.h


def maxch(L, d):
    return 1 if (2 * L * (1 + d) + 3) // 4 <= 64 else 2


def fused_families():
    """{(d, MAXCH): [L, ...]} of every shape plx_apply_backward accepts, from the Python predicate."""
    fam = {}
    for d in range(1, 33):
        for L in range(1, 65):
            if plx.Lattice.backward_fusable(L, d):
                fam.setdefault((d, maxch(L, d)), []).append(L)
    return fam


FAMILIES = fused_families()
FUSED_D = sorted({d for d, _ in FAMILIES})


def band_ends(d):
    """The smallest and the largest L of each family at this d (the 64 / 65-chunk switch lies between two of them)."""
    return sorted({f(Ls) for (dd, _), Ls in FAMILIES.items() if dd == d for f in (min, max)})


_DK = {}


def deriv_taps(profile="rbf", order=1):
    key = (profile, order)
    if key not in _DK:
        fn = plx.rbf if profile == "rbf" else (lambda d2: plx.Matern.apply(d2, 1.5))
        _DK[key] = plx.DiscretizedKernelFN(fn, order)
    return _DK[key].get_deriv_coeffs().numpy()


WORST = {}        # (d, MAXCH) -> [grad_x / ||T||, grad_x rel-L2, grad_src rel-L2, forward rel-L2]; other shapes: (d, L)


def record(d, L, i, value):
    if value is None:
        return
    key = (d, maxch(L, d)) if plx.Lattice.backward_fusable(L, d) else ("other", d, L)
    row = WORST.setdefault(key, [0.0, 0.0, 0.0, 0.0])
    row[i] = max(row[i], value)


@pytest.fixture(scope="module", autouse=True)
def family_report():
    yield
    if not WORST:
        return
    print(f"\nfused backward vs float64, worst per family (bars: grad_x {TAU:.1e} of ||T||, rel {REL_X:.1e}; "
          f"grad_src / forward rel {REL:.1e})")
    print(f"{'d':>3} {'MAXCH':>5} {'L':>7}  {'kernel':>8}  {'gx/|T|':>8} {'gx rel':>8} {'gsrc rel':>8} {'fwd rel':>8}")
    for (d, mc), Ls in sorted(FAMILIES.items()):
        w = WORST.get((d, mc))
        kern = "compiled" if d <= 20 else "run-time"
        cells = " ".join(f"{v:8.1e}" for v in w) if w else "  (not run)"
        print(f"{d:3d} {mc:5d} {min(Ls):3d}..{max(Ls):<2d}  {kern:>8}  {cells}")
    for key in sorted(k for k in WORST if k[0] == "other"):
        print(f"not fused, d = {key[1]}, L = {key[2]}:", " ".join(f"{v:8.1e}" for v in WORST[key]))
    fam = [w for k, w in WORST.items() if k[0] != "other"]
    worst = [max(w[i] for w in fam) for i in range(4)]
    print("overall worst:", " ".join(f"{v:.2e}" for v in worst), f"({len(fam)} of {len(FAMILIES)} families run)")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def check_backward(d, L, gx, gs, want, what):
    gx64, gs64, T = want
    terms, rel = grad_x_ratios(gx.cpu().numpy(), gx64, T)
    record(d, L, 0, terms)
    record(d, L, 1, rel)
    assert terms <= TAU, (what, "grad_x / ||T||", terms)
    assert rel is None or rel <= REL_X, (what, "grad_x rel-L2", rel)
    if gs is not None:
        e = rel_l2(gs.cpu().numpy(), gs64)
        record(d, L, 2, e)
        assert e <= REL, (what, "grad_src rel-L2", e)


def torch_stack(g, s, x):
    """[g | g (x) x | src | src (x) x] in fp32, as LatticeFilterGeneral.backward forms it (py:113-119)."""
    n, L = g.shape
    gx = (g[:, :, None] * x[:, None, :]).reshape(n, -1)
    sx = (s[:, :, None] * x[:, None, :]).reshape(n, -1)
    return torch.cat([g, gx, s, sx], dim=1).contiguous()


def run_family_case(d, L, x, lat64, hip, G, S, what, forward=True):
    """One (d, L) on one lattice: the fused call against backward64, and the forward product of the stacked matrix."""
    g, s = np.ascontiguousarray(G[:, :L]), np.ascontiguousarray(S[:, :L])
    f64 = lat64.apply(stack64(g, s, x))
    want = contract64(g, s, x, f64)
    gc, sc, xc = cuda(g), cuda(s), cuda(x)
    gx, gs = hip.apply_backward(gc, sc, xc)
    check_backward(d, L, gx, gs, want, what)
    if forward:
        got = hip.apply(torch_stack(gc, sc, xc)).cpu().numpy()
        e = rel_l2(got, f64)
        record(d, L, 3, e)
        assert e <= REL, (what, "forward of the stack, rel-L2", e)
    return want, (gc, sc, xc), (gx, gs)


@pytest.mark.parametrize("d", FUSED_D)
def test_every_fused_family_matches_fp64(d):
    """Every (d, MAXCH) family at both ends of its L band, on five clouds; on the densest cloud also the run-time kernel
    for d <= 20 (contract_v = 0), the lattice row order and determinism."""
    taps = deriv_taps()
    Ls = band_ends(d)
    lib = nv.lib()
    for kind in CLOUDS:
        x = cloud(kind, N, d, seed=d, coeffs=taps)
        lat64 = Lattice64(x, taps)
        rng = np.random.default_rng(1000 + d)
        G = rng.standard_normal((N, max(Ls))).astype(np.float32)
        S = rng.standard_normal((N, max(Ls))).astype(np.float32)
        hip = plx.Lattice().build(cuda(x), taps)
        try:
            for L in Ls:
                want, (gc, sc, xc), (gx, gs) = run_family_case(d, L, x, lat64, hip, G, S, (kind, d, L))
                if kind != "gauss0.3":
                    continue
                # determinism: a second call gives the same bits
                gx2, gs2 = hip.apply_backward(gc, sc, xc)
                assert torch.equal(gx, gx2) and torch.equal(gs, gs2), (d, L)
                # lattice row order: the kernels' perm == nullptr path
                perm = torch.from_numpy(hip.export(nv.ARRAY_POINT_PERM).astype(np.int64)).cuda()
                hip.set_lattice_row_order(True)
                try:
                    lx, ls = hip.apply_backward(gc[perm].contiguous(), sc[perm].contiguous(), xc[perm].contiguous())
                finally:
                    hip.set_lattice_row_order(False)
                ux, us = torch.empty_like(lx), torch.empty_like(ls)
                ux[perm], us[perm] = lx, ls
                check_backward(d, L, ux, us, want, ("lattice rows", d, L))
            if kind == "gauss0.3" and d <= 20:
                # the run-time slice_contract_kernel for the families the compiled one serves
                assert lib.plx_tune(b"contract_v", 0) == 0
                try:
                    hip.build(cuda(x), taps)
                finally:
                    assert lib.plx_tune(b"contract_v", 1) == 0
                for L in Ls:
                    run_family_case(d, L, x, lat64, hip, G, S, ("contract_v = 0", d, L), forward=False)
        finally:
            hip.close()


@pytest.mark.parametrize("n", [1, 3, 65, 257])
def test_fused_families_at_partial_waves(n):
    """Few points: partial waves (one point per wave, four waves per workgroup) and a single partial workgroup."""
    taps = deriv_taps()
    for d in FUSED_D:
        x = cloud("gauss0.3", n, d, seed=d)
        lat64 = Lattice64(x, taps)
        Ls = band_ends(d)
        rng = np.random.default_rng(n + d)
        G = rng.standard_normal((n, max(Ls))).astype(np.float32)
        S = rng.standard_normal((n, max(Ls))).astype(np.float32)
        hip = plx.Lattice().build(cuda(x), taps)
        try:
            for L in Ls:
                run_family_case(d, L, x, lat64, hip, G, S, ("n", n, d, L), forward=False)
        finally:
            hip.close()


@pytest.mark.parametrize("d", [2, 3, 5, 8, 13, 20, 21, 26, 32])
def test_fused_families_matern_order3(d):
    """Matern-1.5 at order 3: seven derivative taps, which differ from the forward ones."""
    taps = deriv_taps("matern15", 3)
    Ls = band_ends(d)
    for kind in ("gauss0.3", "isolated"):
        x = cloud(kind, N, d, seed=50 + d, coeffs=taps)
        lat64 = Lattice64(x, taps)
        rng = np.random.default_rng(2000 + d)
        G = rng.standard_normal((N, max(Ls))).astype(np.float32)
        S = rng.standard_normal((N, max(Ls))).astype(np.float32)
        hip = plx.Lattice().build(cuda(x), taps)
        try:
            for L in Ls:
                run_family_case(d, L, x, lat64, hip, G, S, ("matern", kind, d, L))
        finally:
            hip.close()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("d,L", [(1, 3), (1, 30), (32, 1), (2, 40), (30, 20)])
def test_three_call_form_matches_fp64(d, L):
    """plx_backward_stack + apply + plx_backward_contract on shapes the fused call refuses: the stack is the fp32 torch
    products bit for bit, the contraction is the float64 one of the same filtered input, the chain is backward64."""
    assert not plx.Lattice.backward_fusable(L, d)
    taps = deriv_taps()
    lib = nv.lib()
    for kind in ("gauss0.3", "isolated"):
        x = cloud(kind, N, d, seed=d, coeffs=taps)
        rng = np.random.default_rng(3 * d + L)
        g = rng.standard_normal((N, L)).astype(np.float32)
        s = rng.standard_normal((N, L)).astype(np.float32)
        gc, sc, xc = cuda(g), cuda(s), cuda(x)
        W = 2 * L * (1 + d)
        stacked = torch.empty((N, W), dtype=torch.float32, device="cuda")
        nv.check(lib.plx_backward_stack(_ptr(gc), _ptr(sc), _ptr(xc), N, L, d, _ptr(stacked), _stream()), "stack")
        assert torch.equal(stacked, torch_stack(gc, sc, xc))
        hip = plx.Lattice().build(xc, taps)
        try:
            filtered = hip.apply(stacked)
        finally:
            hip.close()
        grad = torch.empty((N, d), dtype=torch.float32, device="cuda")
        nv.check(lib.plx_backward_contract(_ptr(gc), _ptr(sc), _ptr(xc), _ptr(filtered), N, L, d, _ptr(grad), _stream()),
                 "contract")
        # the contraction alone: float64 from the same filtered input
        same = contract64(g, s, x, filtered.cpu().numpy())
        terms, _ = grad_x_ratios(grad.cpu().numpy(), same[0], same[2])
        print(f"three-call form d = {d}, L = {L}, {kind}: contraction alone {terms:.1e} of ||T||")
        assert terms <= TAU, (kind, "contraction", terms)
        # the whole chain
        lat64 = Lattice64(x, taps)
        f64 = lat64.apply(stack64(g, s, x))
        e = rel_l2(filtered.cpu().numpy(), f64)
        record(d, L, 3, e)
        assert e <= REL, (kind, "forward of the stack", e)
        check_backward(d, L, grad, filtered[:, :L], contract64(g, s, x, f64), ("three-call", kind, d, L))


@pytest.mark.parametrize("profile,order,d,L", [("rbf", 1, 8, 11), ("rbf", 1, 21, 5), ("rbf", 1, 3, 20), ("rbf", 1, 32, 7),
                                               ("rbf", 1, 1, 3), ("rbf", 1, 32, 1), ("rbf", 1, 4, 2),
                                               ("matern15", 3, 8, 11), ("matern15", 3, 2, 40)])
def test_autograd_gradients_match_fp64(profile, order, d, L):
    """LatticeFilterGeneral.apply with fused_backward True and False: x.grad, v.grad and the output against float64."""
    fn = plx.rbf if profile == "rbf" else (lambda d2: plx.Matern.apply(d2, 1.5))
    dk = plx.DiscretizedKernelFN(fn, order)
    x = cloud("gauss0.3", N, d, seed=d)
    rng = np.random.default_rng(d * L)
    v = rng.standard_normal((N, L)).astype(np.float32)
    w = rng.standard_normal((N, L)).astype(np.float32)
    fwd64 = Lattice64(x, dk.get_coeffs().numpy()).apply(v)
    lat64 = Lattice64(x, dk.get_deriv_coeffs().numpy())
    want = contract64(w, v, x, lat64.apply(stack64(w, v, x)))
    assert plx.LatticeFilterGeneral.method is None and plx.LatticeFilterGeneral.fused_backward
    try:
        for fused in (True, False):
            plx.LatticeFilterGeneral.fused_backward = fused
            xt = cuda(x).requires_grad_(True)
            vt = cuda(v).requires_grad_(True)
            out = plx.LatticeFilterGeneral.apply(vt, xt, dk)
            (out * cuda(w)).sum().backward()
            e = rel_l2(out.detach().cpu().numpy(), fwd64)
            record(d, L, 3, e)
            assert e <= REL, ("autograd forward", fused, profile, d, L, e)
            check_backward(d, L, xt.grad, vt.grad, want, ("autograd", fused, profile, d, L))
    finally:
        plx.LatticeFilterGeneral.fused_backward = True
        plx.lattice_cache().clear()


def test_acceptance_agrees_with_backward_fusable():
    """plx_apply_backward returns 0 exactly where Lattice.backward_fusable says so, PLX_ERR_INVALID elsewhere, and a
    refused call leaves the lattice usable (d = 1..32, L = 1..64 on a tiny lattice)."""
    lib = nv.lib()
    taps = deriv_taps()
    n = 5
    rng = np.random.default_rng(0)
    for d in range(1, 33):
        x = cloud("gauss1", n, d, seed=d)
        xc = cuda(x)
        hip = plx.Lattice().build(xc, taps)
        try:
            grad_x = torch.empty((n, d), dtype=torch.float32, device="cuda")
            for L in range(1, 65):
                g = cuda(rng.standard_normal((n, L)))
                grad_s = torch.empty((n, L), dtype=torch.float32, device="cuda")
                rc = lib.plx_apply_backward(hip._h, _ptr(g), _ptr(g), _ptr(xc), L, _ptr(grad_x), _ptr(grad_s), _stream())
                if plx.Lattice.backward_fusable(L, d):
                    assert rc == 0, (d, L, rc, lib.plx_last_error())
                    assert torch.isfinite(grad_x).all() and torch.isfinite(grad_s).all()
                else:
                    assert rc == PLX_ERR_INVALID, (d, L, rc)
            v = rng.standard_normal((n, 3)).astype(np.float32)
            assert rel_l2(hip.apply(cuda(v)).cpu().numpy(), Lattice64(x, taps).apply(v)) <= REL
        finally:
            hip.close()
    torch.cuda.synchronize()
