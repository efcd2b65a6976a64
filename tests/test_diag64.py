"""The identity behind the native diagonal (csrc/plx_diag_kernels.h), pinned on the CPU before any HIP runs:

    K_ii = (1 / (1 + 2^-d)) sum_{a,b} w_a w_b sum_c prod_j tap[c + s_j(a, b)]     (tests/diag64.py)

tests/diag64.diag_paths forms it from the oracle's tables alone -- corners, weights, the neighbour table -- and must
reproduce the diagonal of the dense float64 matrix to 8 * 2^-52 * diag_terms at every entry.  The same sum carried in
numpy float32 must meet the bar the fp32 kernel is held to on the GPU, k * 2^-24 * diag_terms with
k = (d+1)^2 (2r+1) + d + 4: that bar is satisfiable by a plain sequential fp32 sum.  No GPU.
"""
import numpy as np
import pytest

from tests import diag64
from tests.lattice64 import Lattice64, cloud
from tests.sym64 import taps_of

CLOUDS = ("gauss1", "simplex", "isolated", "dup", "grid")
DIMS = (1, 2, 3, 8)
ORDERS = (0, 1, 2, 3)


def _n_of(kind, d):
    return {"gauss1": 300, "simplex": 120, "isolated": 64, "dup": 300, "grid": 300}[kind] - 7 * (d == 8)


@pytest.mark.parametrize("lopsided", [False, True], ids=["sym", "lopsided"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", CLOUDS)
def test_paths_reproduce_the_dense_diagonal(kind, d, order, lopsided):
    taps = taps_of(order, lopsided)
    x = cloud(kind, _n_of(kind, d), d, seed=1, coeffs=taps)
    L = Lattice64(x, taps)
    dense, terms = diag64.diag_dense(L), diag64.diag_terms(L)
    assert np.all(terms > 0), "w_a^2 c_r^(d+1) > 0 for some corner of every point"
    got, nesting_is_rank = diag64.diag_paths(x, taps, return_rank_check=True)
    assert nesting_is_rank, "the axis nesting read from the neighbour table is the one of the rank permutation"
    r64 = float((np.abs(got - dense) / terms).max())
    got32 = diag64.diag_paths(x, taps, dtype=np.float32)
    assert got32.dtype == np.float32
    r32 = float((np.abs(got32.astype(np.float64) - dense) / terms).max())
    k = diag64.bar_terms(d, order)
    print(f"{kind} d={d} order={order} lopsided={lopsided}: float64 {r64 / 2.0 ** -52:.2f} of 8 ulp64, "
          f"float32 {r32 / 2.0 ** -24:.2f} of {k} ulp32")
    assert r64 <= 8 * 2.0 ** -52, r64
    assert r32 <= k * 2.0 ** -24, r32


def test_order_zero_is_the_closed_form():
    """ntaps = 1: c_0^(d+1) sum_a w_a^2 / (1 + 2^-d), through the same code."""
    d = 3
    taps = np.array([0.8], np.float32)
    x = cloud("gauss1", 200, d, seed=2)
    L = Lattice64(x, taps)
    from oracle import oracle
    oracle.set_exact_mode(False)
    try:
        lat = oracle.Lattice(x, taps)
    finally:
        oracle.set_exact_mode(True)
    w = lat.entry_weight.astype(np.float64)
    lat.close()
    want = float(np.float32(0.8)) ** (d + 1) * (w * w).sum(1) / (1 + 2.0 ** -d)
    # (distinct corners of one simplex are distinct vertices, so S S^T has exactly sum_a w_a^2 on its diagonal)
    np.testing.assert_allclose(diag64.diag_paths(x, taps), want, rtol=1e-14)
    np.testing.assert_allclose(diag64.diag_dense(L), want, rtol=1e-14)


def test_the_diagonal_is_not_one():
    """What the feature is for: at d = 8 the declared unit diagonal is about three times the operator's."""
    taps = taps_of(1, False)
    x = cloud("gauss1", 293, 8, seed=1)
    dd = diag64.diag_dense(Lattice64(x, taps))
    assert 0.2 < dd.min() and dd.max() < 0.7 and dd.mean() < 0.45
