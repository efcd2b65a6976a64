"""tests/query_grad64 on the CPU: the yardstick of the query position gradient pinned against itself and against central
differences of the yardstick of the query route (tests/query64.Query64.apply64).

At d in {1, 2, 3, 8, 18}, n = 300, nq = 32 jittered queries:

  1. the geometric Jacobian (a linear solve on the corner keys, no rank) and the closed form the device uses (rank
     permutation and scale factors) agree to 1e-12 relative;
  2. central differences of apply64 at an fp32-representable step h agree with J^T values on the (query, axis) pairs whose
     x + h e_j and x - h e_j keep all d + 1 corner keys, under the bar derived below;
  3. a condition on the inputs: at least half of the pairs are kept in every case.

The bar of 2.  On a kept pair the three points lie in one simplex, where the weights float64 gives, w64, are affine: their
central difference IS J, exactly.  apply64 does not use w64 but the oracle's fp32 weights w32 (converted exactly), so

    CD - J^T values / denom = sum_r [(w32 - w64)_r(x + h e_j) - (w32 - w64)_r(x - h e_j)] values_r / (2 h' denom)

with h' the step actually taken ((x + h) - (x - h) in fp32, divided by exactly), and therefore

    |CD - J^T values / denom| <= c 2^-24 sum_r |values_r| / (h' denom),    c = max |w32 - w64| / 2^-24

over the corners of the shifted queries of the case.  c is the reference's own error: the fp32 weights of the oracle against
the float64 solution of sum_r w_r P_r = E x, sum_r w_r = 1 on the oracle's own corner keys (query_grad64.weight_error) -- it
involves neither Jacobian.  A worst-case count of the roundings of the embedding (2 (d - i) + 4 on the terms of el_i, whose
sizes add up to several cells, three more on the scaled difference, one on the difference of two of them) bounds c by
some thousands at d = 18 and is of no use as a bar; measured from the reference, c is 1.6, 3.7, 5.3, 6.3 and 26 at the five
d (printed), and the worst difference is 0.91 to 1.75 times 2^-24 sum_r |values_r| / (h denom).  The float64 arithmetic of
both sides adds 64 2^-52 sum_r |values_r| / h', which is included.  So that a regression of the oracle's weights cannot
widen the bar unseen, c itself is held under that a-priori count (query_grad64.weight_error_cap, derived there from the
positions and the scale factors alone): c <= 2 (2 d + 4) A / (d + 1) + 10.
"""
import numpy as np
import pytest

from tests.lattice64 import Lattice64, cloud
from tests.query_grad64 import U24, QueryGrad64, shifted, weight_error, weight_error_cap
from tests.sym64 import taps_of

DS = (1, 2, 3, 8, 18)
N, NQ, VD = 300, 32, 3
H = 2.0 ** -7                                  # fp32-representable; the kept share at d = 18 is 0.585 with it
_CASES = {}


def case(d):
    """(X, taps, Lattice64, queries, h, base Query64, plus, minus, kept, QueryGrad64), computed once per d."""
    if d not in _CASES:
        order = (1, 2, 3, 1, 3)[DS.index(d)]
        taps = taps_of(order, False)
        X = cloud("gauss1", N, d, seed=d + order, coeffs=taps)
        L = Lattice64(X, taps)
        rng = np.random.default_rng(100 + d + order)
        Q = (X[:NQ] + 0.05 * rng.standard_normal((NQ, d))).astype(np.float32)
        h = H
        base, plus, minus, kept = shifted(X, Q, taps, h, L)
        _CASES[d] = (X, taps, L, Q, h, base, plus, minus, kept, QueryGrad64(base, taps))
    return _CASES[d]


@pytest.mark.parametrize("d", DS)
def test_the_two_jacobians_agree(d):
    *_, G = case(d)
    scale = np.abs(G.J_geo).max()
    err = np.abs(G.J - G.J_geo).max() / scale
    print(f"d = {d}: closed form against the geometric solve: {err:.2e} relative")
    assert err <= 1e-12, err
    # the weights sum to one whatever the position: the columns of J sum to zero over the corners
    assert np.abs(G.J_geo.sum(1)).max() <= 1e-12 * scale
    # grad64 (geometric) and the pull-back of dots64 (closed form) are the same map
    values = np.random.default_rng(d).standard_normal((G.ref.m, VD))
    g = np.random.default_rng(d + 1).standard_normal((G.nq, VD))
    t, T = G.dots64(values, g)
    assert np.abs(G.pull(t) - G.grad64(values, g)).max() <= 1e-12 * G.terms(T).max()
    assert (t[~G.ref.found] == 0).all()


@pytest.mark.parametrize("d", DS)
def test_at_least_half_of_the_pairs_are_kept(d):
    """A condition on the inputs, from the reference alone."""
    *_, kept, _ = case(d)
    print(f"d = {d}: h = {H}, kept share {kept.mean():.3f}")
    assert kept.mean() >= 0.5, kept.mean()


@pytest.mark.parametrize("d", DS)
def test_central_differences_of_apply64(d):
    X, taps, L, Q, h, base, plus, minus, kept, G = case(d)
    v = np.random.default_rng(7 + d).standard_normal((N, VD))
    values = base.blurred64(v)
    want = G.jacobian_apply(values)                                           # [nq, vd, d]
    S = np.abs(G.corner_rows(values)).sum(1) / base.denom                     # [nq, vd]: sum_r |values_r| / denom
    c, worst = 0.0, 0.0
    cap = 0.0
    for j in range(d):
        (Qp, rp), (Qm, rm) = plus[j], minus[j]
        c = max(c, weight_error(rp, G.E, Qp), weight_error(rm, G.E, Qm))
        cap = max(cap, weight_error_cap(G.s, Qp), weight_error_cap(G.s, Qm))
    assert c <= cap, (c, cap, "the reference's fp32 weights are further from float64 than their roundings allow")
    for j in range(d):
        (Qp, rp), (Qm, rm) = plus[j], minus[j]
        step = Qp[:, j].astype(np.float64) - Qm[:, j].astype(np.float64)      # 2 h'
        cd = (rp.apply64(v) - rm.apply64(v)) / step[:, None]
        bar = (c * U24 + 64 * 2.0 ** -52) * S / (step[:, None] / 2)
        k = kept[:, j]
        if k.any():
            err = np.abs(cd - want[:, :, j])[k]
            assert not err[bar[k] == 0].any()                                 # no corner found: both sides are exactly 0
            worst = max(worst, (err[bar[k] > 0] / bar[k][bar[k] > 0]).max(initial=0.0))
    print(f"d = {d}: h = {h}, c = {c:.2f} (cap {cap:.0f}), kept {kept.mean():.3f}, worst share of the bar {worst:.3f}; "
          f"in units of 2^-24 sum |values_r| / h: {worst * c:.2f}")
    assert worst <= 1.0, worst
