"""tests/query64 on the CPU: the yardstick of the query route pinned against the yardstick of the product.

  * At queries that ARE rows of X the reference is the rows of Lattice64(X): ids and weights array-equal to X's own, the
    product equal to the same rows of Lattice64(X).apply, exactly (the same sparse matrices in the same order).
  * Far queries give zero rows and zero mass.
  * The conditions tests/test_query_gpu.py puts on its inputs hold for the reference alone: the found share of the `jit`
    queries stays between 50 % and 100 % at d <= 8, and at every d >= 2 some `jit` case has an absent corner.
"""
import numpy as np
import pytest

from oracle import oracle
from tests.lattice64 import Lattice64, cloud
from tests.query64 import Query64, _structure
from tests.sym64 import taps_of


@pytest.mark.parametrize("d", [1, 2, 3, 8, 18])
@pytest.mark.parametrize("order", [0, 1, 3])
def test_train_queries_are_rows_of_the_lattice(d, order):
    n, nq = 300, 120
    taps = taps_of(order, False)
    X = cloud("gauss1", n, d, seed=d + order, coeffs=taps)
    L = Lattice64(X, taps)
    q = Query64(X, X[:nq], taps, lattice=L)
    _, ev, ew = _structure(X, taps)
    assert np.array_equal(q.vid, ev[:nq]) and np.array_equal(q.weight, ew[:nq])
    assert q.found.all() and q.found_share == 1.0
    v = np.random.default_rng(d).standard_normal((n, 3))
    assert np.array_equal(q.apply64(v), L.apply_staged(v)[:nq])
    assert np.array_equal(q.terms64(v), L.terms64(v)[:nq])
    # the whole simplex found: the mass is the fp32 sum of all d + 1 weights, 1 to rounding (per weight: the scaled
    # difference it is, at most three roundings of numbers below 1, and one addition)
    assert q.mass32.dtype == np.float32 and np.abs(q.mass32 - 1.0).max() <= 4 * (d + 1) * 2.0 ** -24


@pytest.mark.parametrize("d,order", [(1, 1), (3, 2), (8, 3)])
def test_far_queries_give_zero(d, order):
    taps = taps_of(order, True)
    X = cloud("gauss1", 200, d, seed=1, coeffs=taps)
    sf = oracle.scale_factors(d, taps)
    far = X[:50].copy()
    far[:, 0] += 12.0 * d * 40 / float(sf[0])                  # far beyond the cloud, well inside the int16 keys
    q = Query64(X, far, taps)
    assert not q.found.any() and q.found_share == 0.0
    v = np.random.default_rng(0).standard_normal((200, 2))
    assert not q.apply64(v).any() and not q.terms64(v).any() and not q.mass32.any()
    assert q.S_Q.nnz == 0


def test_jitter_found_share_is_in_the_regime():
    """gauss1, n = 300, X + 0.05 N(0, 1): between 50 % and 100 % of the corners found at d <= 8, an absent corner at
    every d >= 2, fewer found at d = 18."""
    shares = {}
    for d in (1, 2, 3, 8, 18):
        for order in (0, 1, 3):
            taps = taps_of(order, False)
            X = cloud("gauss1", 300, d, seed=d + order, coeffs=taps)
            rng = np.random.default_rng(100 + d + order)
            Q = (X[:200] + 0.05 * rng.standard_normal((200, d))).astype(np.float32)
            shares[d, order] = Query64(X, Q, taps).found_share
    print({k: round(v, 3) for k, v in shares.items()})
    for (d, order), s in shares.items():
        if d <= 8:
            assert 0.5 <= s <= 1.0, (d, order, s)
    for d in (2, 3, 8, 18):
        assert min(shares[d, o] for o in (0, 1, 3)) < 1.0, d
    assert max(shares[18, o] for o in (0, 1, 3)) < 1.0
