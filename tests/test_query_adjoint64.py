"""tests/query_adjoint64 pinned on the CPU (no GPU): the adjoint identity against Query64.apply64, the splat at Q = X against
Lattice64's own S^T, and the conditions on the inputs of tests/test_query_adjoint_gpu.py, from the reference alone.
Fails without the feature (the helper is part of it)."""
import numpy as np
import pytest

from tests.lattice64 import Lattice64, cloud
from tests.query64 import Query64
from tests.query_adjoint64 import ALL_ABSENT, DEPTH_CASE, SINGLE, SPLAT_CASES, SPLAT_SETS, QueryAdjoint64
from tests.sym64 import taps_of

DS = (1, 2, 3, 8, 18)


def _pair(d, order=1):
    taps = taps_of(order, False)
    X = cloud("gauss1", 300, d, seed=3 + d, coeffs=taps)
    Q = (X[:32] + 0.05 * np.random.default_rng(7 + d).standard_normal((32, d))).astype(np.float32)
    return X, Q, taps


@pytest.mark.parametrize("d", DS)
def test_the_adjoint_identity(d):
    """<apply64(v), g> == <v, apply_t64(g)> to 1e-12 relative."""
    X, Q, taps = _pair(d)
    ref = Query64(X, Q, taps)
    A = QueryAdjoint64(ref)
    rng = np.random.default_rng(d)
    for vd in (1, 3):
        v, g = rng.standard_normal((300, vd)), rng.standard_normal((32, vd))
        lhs = float((ref.apply64(v) * g).sum())
        rhs = float((v * A.apply_t64(g)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (d, vd, lhs, rhs)
        assert (np.abs(A.apply_t64(g)) <= A.terms_t64(g) * (1 + 1e-12)).all()


@pytest.mark.parametrize("d", DS)
def test_the_splat_at_the_build_points_is_the_builds(d):
    """splat_at64 at Q = X equals Lattice64.S.T @ g; the counts are the build's vertex row lengths."""
    X, _, taps = _pair(d)
    L = Lattice64(X, taps)
    ref = Query64(X, X, taps, lattice=L)
    assert ref.found.all()
    A = QueryAdjoint64(ref)
    g = np.random.default_rng(2 * d).standard_normal((300, 3))
    want = L.S.T @ g
    got = A.splat_at64(g).astype(np.float64)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(A.splat_terms64(g)).max()
    assert A.counts.sum() == 300 * (d + 1) and A.cmax == A.counts.max()
    # another numbering permutes the rows
    perm = np.random.default_rng(1).permutation(ref.m)
    P = QueryAdjoint64(ref, id_of=perm)
    assert np.array_equal(P.splat_at64(g)[perm], A.splat_at64(g)) and np.array_equal(P.counts[perm], A.counts)
    assert np.array_equal(P.apply_t64(g), A.apply_t64(g))


def test_the_inputs_of_the_gpu_contracts_hold_their_conditions():
    """Every (case, query set) of the per-entry contract: a vertex with no query corner; a vertex with two or more, or the
    stated reason why not (query_adjoint64.SINGLE / ALL_ABSENT); for jit at d >= 8 a found share strictly inside (0, 1)."""
    from tests.test_query_gpu import CASES, reference
    shown = {}
    for key in SPLAT_CASES + [DEPTH_CASE]:
        assert key in CASES, key
        for name in SPLAT_SETS:
            ref = reference(key, name)
            A = QueryAdjoint64(ref)
            touched = float((A.counts > 0).mean())
            shown[key[:3] + (name,)] = (round(ref.found_share, 2), round(touched, 2), A.cmax)
            if name == "far" or (key, name) in ALL_ABSENT:
                assert not ref.found.any() and A.cmax == 0, (key, name)
                continue
            if key == DEPTH_CASE:
                assert A.cmax >= 100, (key, name, A.cmax)                 # the long sums; every vertex may be touched
            else:
                assert (A.counts == 0).any(), (key, name, "a vertex with no query corner")
            if (key, name) in SINGLE:
                assert A.cmax == 1, (key, name, A.cmax)
            else:
                assert A.cmax >= 2, (key, name, A.cmax)
            if name == "jit" and key[1] >= 8:
                assert 0.0 < ref.found_share < 1.0, (key, ref.found_share)
    print(shown)


def test_the_power_of_two_lattice():
    """m = 8: the absent key m needs one bit more than the ids up to m - 1."""
    taps = taps_of(1, False)
    L = Lattice64(cloud("gauss1", 300, 1, seed=5, coeffs=taps), taps)
    assert L.m == 8
