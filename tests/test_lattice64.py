"""The float64 lattice operator (tests/lattice64.py) is the same operation as the fp32 CPU oracle before it judges the HIP
kernels: K64 against oracle.filter, backward64 against the reference formulation (py:113-123) over the oracle.  CPU only."""
import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from oracle import oracle
from tests.lattice64 import Lattice64, backward64, cloud, contract64, entry_ratio, grad_x_ratios, rel_l2, stack64

PROFILES = {"rbf": plx.rbf, "matern15": lambda d2: plx.Matern.apply(d2, 1.5)}
_TAPS = {}


def taps(profile, order, deriv=False):
    key = (profile, order)
    if key not in _TAPS:
        _TAPS[key] = plx.DiscretizedKernelFN(PROFILES[profile], order)
    dk = _TAPS[key]
    return (dk.get_deriv_coeffs() if deriv else dk.get_coeffs()).numpy()


def oracle_filter(src, ref, coeffs):
    oracle.set_exact_mode(False)
    try:
        return oracle.filter(src, ref, coeffs)
    finally:
        oracle.set_exact_mode(True)


@pytest.mark.parametrize("d", range(1, 33))
def test_k64_is_the_oracle_filter(d):
    """K64 v == oracle.filter(v) (fp32, exact mode off) to rel-L2 1e-6: every d, taps of order 0..3 of two profiles,
    random, duplicate, one-simplex and isolated clouds."""
    rng = np.random.default_rng(d)
    n = 97
    v = rng.standard_normal((n, 3)).astype(np.float32)
    worst = 0.0
    for profile in ("rbf", "matern15"):
        for order in (0, 1, 2, 3):
            c = taps(profile, order)
            for kind in ("gauss0.3", "gauss1", "dup", "simplex", "isolated"):
                x = cloud(kind, n, d, seed=d, coeffs=c)
                lat = Lattice64(x, c)
                if kind == "simplex":
                    assert lat.m == d + 1
                want = oracle_filter(v, x, c)
                got = lat.apply(v)
                err = rel_l2(want, got)
                worst = max(worst, err)
                assert err <= 1e-6, (profile, order, kind, err)
                assert rel_l2(lat.apply_staged(v), got) <= 1e-13
    print(f"d = {d}: K64 vs oracle worst rel-L2 {worst:.2e}")


def test_k64_blur_order_and_absent_neighbours():
    """The neighbour slots are nid = -r..-1, 1..r: asymmetric taps tell the directions apart, and a lattice of one simplex
    (every neighbour outside it absent) still matches the oracle."""
    c = np.array([0.1, 0.3, 1.0, 0.6, 0.2], np.float32)
    for d in (1, 2, 5):
        for kind in ("gauss1", "simplex"):
            x = cloud(kind, 60, d, seed=3)
            v = np.random.default_rng(4).standard_normal((60, 2)).astype(np.float32)
            assert rel_l2(oracle_filter(v, x, c), Lattice64(x, c).apply(v)) <= 1e-6, (d, kind)
            flipped = Lattice64(x, c[::-1].copy()).apply(v)
            if kind == "gauss1":
                assert rel_l2(oracle_filter(v, x, c), flipped) > 1e-3, d


def test_isolated_cloud_has_no_gradient():
    """The isolated cloud is what it claims: every point alone on its d+1 vertices, out of every blur's reach, so the
    true position gradient is 0 to rounding while its terms are not."""
    for d in (1, 2, 3, 8, 21, 32):
        c = taps("matern15", 3, deriv=True)
        x = cloud("isolated", 301, d, coeffs=c)
        lat = Lattice64(x, c)
        assert lat.m == 301 * (d + 1)
        rng = np.random.default_rng(d)
        gx, _, T = backward64(rng.standard_normal((301, 2)), rng.standard_normal((301, 2)), x, c, lattice=lat)
        assert np.linalg.norm(gx) <= 1e-14 * np.linalg.norm(T), d


def torch_backward_over_oracle(dk, x, v, w):
    """LatticeFilterGeneral.backward's fp32 torch formulation (py:113-123) with the oracle as the filter."""
    def method(src, ref, coeffs):
        return torch.from_numpy(oracle_filter(src.detach().numpy(), ref.detach().numpy(), coeffs.detach().numpy()))
    plx.LatticeFilterGeneral.method = staticmethod(method)
    try:
        xt = torch.from_numpy(x).requires_grad_(True)
        vt = torch.from_numpy(v).requires_grad_(True)
        out = plx.LatticeFilterGeneral.apply(vt, xt, dk)
        (out * torch.from_numpy(w)).sum().backward()
    finally:
        plx.LatticeFilterGeneral.method = None
    return out.detach().numpy(), vt.grad.numpy(), xt.grad.numpy()


@pytest.mark.parametrize("profile,order", [("rbf", 1), ("rbf", 2), ("matern15", 3)])
@pytest.mark.parametrize("d,L,scale", [(1, 3, 0.3), (2, 5, 0.3), (3, 2, 1.0), (5, 4, 0.3), (8, 3, 0.3), (12, 2, 0.3),
                                       (20, 2, 0.1), (32, 2, 0.1)])
def test_backward64_is_the_reference_formulation(profile, order, d, L, scale):
    """backward64 against the reference's own arithmetic (fp32 torch over the oracle filter) where the gradient does not
    vanish: the two agree to fp32 rounding, so the fp64 helper computes the same operation."""
    dk = plx.DiscretizedKernelFN(PROFILES[profile], order)
    n = 301
    rng = np.random.default_rng(7 * d + L)
    x = cloud(f"gauss{scale}", n, d, seed=d)
    v = rng.standard_normal((n, L)).astype(np.float32)
    w = rng.standard_normal((n, L)).astype(np.float32)
    out, gv, gx = torch_backward_over_oracle(dk, x, v, w)
    gx64, gs64, T = backward64(w, v, x, dk.get_deriv_coeffs().numpy())
    terms, rel = grad_x_ratios(gx, gx64, T)
    assert rel is not None, "this shape's gradient should not vanish"
    assert rel <= 1e-5 and terms <= 1e-5, (terms, rel)
    assert rel_l2(gv, gs64) <= 1e-6
    assert rel_l2(out, Lattice64(x, dk.get_coeffs().numpy()).apply(v)) <= 1e-6


def test_contract64_by_hand():
    """The contraction's index layout on a 2-point, L = 2, d = 3 case written out term by term."""
    rng = np.random.default_rng(0)
    n, L, d = 2, 2, 3
    g, s, x = rng.standard_normal((n, L)), rng.standard_normal((n, L)), rng.standard_normal((n, d))
    f = rng.standard_normal((n, 2 * L * (1 + d)))
    gx, gs, T = contract64(g, s, x, f)
    st = stack64(g, s, x)
    assert st.shape == (n, 2 * L * (1 + d))
    for p in range(n):
        for k in range(d):
            want = t = 0.0
            for l in range(L):
                wg, ws = f[p, l], f[p, L + L * d + l]
                wgx, wsx = f[p, L + l * d + k], f[p, 2 * L + L * d + l * d + k]
                assert st[p, L + l * d + k] == g[p, l] * x[p, k] and st[p, 2 * L + L * d + l * d + k] == s[p, l] * x[p, k]
                parts = (s[p, l] * x[p, k] * wg, -s[p, l] * wgx, g[p, l] * x[p, k] * ws, -g[p, l] * wsx)
                want += -2 * sum(parts)
                t += 2 * sum(abs(q) for q in parts)
            assert abs(gx[p, k] - want) <= 1e-12 and abs(T[p, k] - t) <= 1e-12
    assert np.array_equal(gs, f[:, :L])


def taps_of_order(order, asym=False):
    """2 * order + 1 taps: a Gaussian profile, or (asym) a lopsided one with a centre tap other than 1."""
    half = np.exp(-0.5 * (np.arange(1, order + 1) * 0.7) ** 2)
    if not asym:
        return np.concatenate([half[::-1], [1.0], half]).astype(np.float32)
    return np.concatenate([0.6 * half[::-1], [0.8], 1.1 * half]).astype(np.float32)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 8, 17, 32])
def test_terms64_bounds_the_product(d):
    """|K64 v| <= terms64(v) for signed v, equality (to rounding) for non-negative v (the taps are positive)."""
    rng = np.random.default_rng(40 + d)
    n = 83
    for order, c in ((0, np.array([0.7], np.float32)), (1, taps_of_order(1)), (2, np.array([0.2, 0.5, 1.0, 0.4, 0.1], np.float32)),
                     (3, taps_of_order(3, asym=True))):
        for kind in ("gauss0.3", "gauss1", "simplex", "isolated"):
            x = cloud(kind, n, d, seed=d, coeffs=c)
            lat = Lattice64(x, c)
            v = rng.standard_normal((n, 4))
            T = lat.terms64(v)
            assert T.shape == (n, 4)
            assert np.all(np.abs(lat.apply(v)) <= T * (1 + 1e-12) + 1e-300), (order, kind)
            a = np.abs(v)
            assert np.allclose(lat.terms64(a), lat.apply(a), rtol=1e-12, atol=0), (order, kind)


def test_entry_ratio():
    """Per entry, in units of the entry's own terms; an entry with no terms must be exactly 0."""
    want = np.array([[1.0, 0.0], [-2.0, 0.0]])
    T = np.array([[2.0, 0.0], [4.0, 1.0]])
    assert entry_ratio(want, want, T) == 0.0
    got = want + np.array([[1e-6, 0.0], [0.0, 3e-7]])
    assert entry_ratio(got, want, T) == pytest.approx(5e-7)
    assert entry_ratio(want + np.array([[0.0, 1e-30], [0.0, 0.0]]), want, T) == float("inf")
    assert entry_ratio(np.array([[np.nan, 0.0], [-2.0, 0.0]]), want, T) == float("inf")


@pytest.mark.parametrize("order", range(9))
def test_k64_columns_are_the_oracle_on_one_hot_inputs(order):
    """Column j of K64 is oracle.filter of the j-th unit vector, for every order the ABI takes (0..8): order 0 has no
    neighbour table at all, orders 5..8 have 10..16 neighbour slots per axis.  Symmetric and lopsided taps."""
    for d, kind in ((1, "gauss1"), (2, "gauss0.3"), (3, "gauss1"), (6, "gauss0.3"), (3, "simplex")):
        for asym in (False, True):
            c = taps_of_order(order, asym)
            n = 40
            x = cloud(kind, n, d, seed=order + d, coeffs=c)
            lat = Lattice64(x, c)
            cols = np.array([0, 1, n // 2, n - 1])
            e = np.zeros((n, cols.size), np.float32)
            e[cols, np.arange(cols.size)] = 1.0
            want = oracle_filter(e, x, c).astype(np.float64)
            got = lat.matrix()[:, cols]
            assert entry_ratio(got, want, lat.terms64(e)) <= 1e-6, (order, d, kind, asym)
            assert rel_l2(got, want) <= 1e-6, (order, d, kind, asym)
            assert np.array_equal(lat.apply(e), got)
    # the taps really reach that far: a lopsided order-8 blur differs from its mirror image
    c = taps_of_order(8, asym=True)
    x = cloud("gauss1", 40, 2, seed=1)
    v = np.random.default_rng(0).standard_normal((40, 1))
    assert rel_l2(Lattice64(x, c[::-1].copy()).apply(v), Lattice64(x, c).apply(v)) > 1e-3


def test_forward_families_name_every_kernel_literal():
    """Every kernel family name the sources can report (each string literal assigned to kn_splat / kn_blur / kn_slice in
    simplex_gp_amd/csrc/*.hip) is a stage of some family in tests/test_forward_fp64.FAMILIES, and FAMILIES names nothing
    else: a new family cannot go unchecked.  The empty name (a stage with no owned rows or no corners launches nothing)
    is not a family."""
    import glob
    import os
    import re
    from tests.test_forward_fp64 import FAMILIES, NAMES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    literals = set()
    for path in sorted(glob.glob(os.path.join(root, "simplex_gp_amd", "csrc", "*.hip"))):
        text = open(path).read()
        for stmt in re.finditer(r"\bkn_(?:splat|blur|slice)\s*=([^;]*);", text):
            literals.update(re.findall(r'"([^"]*)"', stmt.group(1)))
    literals.discard("")
    assert len(literals) >= 30
    assert literals == NAMES, {"in the sources only": sorted(literals - NAMES), "in FAMILIES only": sorted(NAMES - literals)}
    assert all(len(f) == 3 for f in FAMILIES)
