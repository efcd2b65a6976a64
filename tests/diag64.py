"""TEST HELPER: the diagonal of the lattice operator, three ways, on top of tests/lattice64.Lattice64.

    diag_dense(L64)          np.diag of the dense float64 matrix K64 = S B_d ... B_0 S^T / (1 + 2^-d);
    diag_terms(L64)          the same diagonal with |S| and |B_j|: the size of the terms each K_ii sums, the yardstick of
                             every bar on the diagonal;
    diag_paths(ref, coeffs)  the construction of csrc/plx_diag_kernels.h restated in numpy from oracle.Lattice, with no
                             matrix at all:

        K_ii = (1 / (1 + 2^-d)) sum_{a,b} w_a w_b (B_d ... B_0)[v_a, v_b]

    An entry of the blur product is a sum over paths of one hop per axis, axis d first, axis 0 last; a hop of shift t in
    [-r, r] goes through the neighbour table (slot t + r below 0, t + r - 1 above) and costs the tap c[t + r]; a path that
    meets an absent neighbour contributes nothing.  The d + 1 blur directions sum to zero and satisfy no other relation, so
    the shift vectors that lead from corner a to corner b of one simplex are t_j = c + s_j with s a fixed 0 / +-1 pattern
    of the pair and c every integer that keeps all t_j in [-r, r].  Corner k - 1 is the +1 neighbour of corner k along
    exactly one axis, j_k: found by looking corner k - 1 up among the +1 neighbours of corner k (pos[j_k] = k; the one axis
    that is no j_k keeps pos 0).  Then for a < b, s_j = -1 where a < pos[j] <= b, and for a > b, s_j = +1 where
    b < pos[j] <= a.

Checker only: the product and the GPU path never import it.
"""
import numpy as np

from oracle import oracle


def diag_dense(L64):
    return np.diag(L64.matrix()).copy()


def diag_terms(L64):
    G = abs(L64.S).T.tocsr()
    for B in L64.blurs:
        G = (abs(B) @ G).tocsr()
    K = abs(L64.S) @ G
    K = K.toarray() if hasattr(K, "toarray") else np.asarray(K)
    return np.diag(K) / L64.denom


def bar_terms(d, r):
    """k of the bars k * eps * diag_terms: one rounding per term of a sequential sum of (d+1)^2 (2r+1) terms, plus the
    roundings of a path's product (d), the two weight products, the division and one to spare."""
    return (d + 1) ** 2 * (2 * r + 1) + d + 4


def axis_positions(ev, nbr, r):
    """pos [n, d+1]: pos[p, j] = k when corner k - 1 of point p is the +1 neighbour of corner k along axis j, else 0."""
    n, d1 = ev.shape
    pos = np.zeros((n, d1), np.int64)
    if r == 0:
        return pos
    found = np.zeros((n, d1), np.int64)
    for k in range(1, d1):
        for j in range(d1):
            hit = nbr[j, r, ev[:, k]] == ev[:, k - 1]          # slot r: shift +1
            pos[hit, j] = k
            found[hit, k] += 1
    assert np.all(found[:, 1:] == 1), "corner k - 1 is the +1 neighbour of corner k along exactly one axis"
    return pos


def diag_paths(ref, coeffs, dtype=np.float64, return_rank_check=False):
    """The diagonal by path sums, every product and sum carried in `dtype`, in the kernel's item order (a, b, c)."""
    ref = np.ascontiguousarray(ref, np.float32)
    c32 = np.ascontiguousarray(np.asarray(coeffs, np.float32).reshape(-1))
    r = c32.size // 2
    oracle.set_exact_mode(False)
    try:
        lat = oracle.Lattice(ref, c32)
    finally:
        oracle.set_exact_mode(True)
    n, d = ref.shape
    d1 = d + 1
    ev = lat.entry_vertex.astype(np.int64)
    ew = lat.entry_weight.astype(dtype)
    rank = lat.rank.astype(np.int64)
    nbr = lat.neighbors().astype(np.int64) if r > 0 else np.empty((d1, 0, int(lat.m)), np.int64)
    lat.close()
    taps = c32.astype(dtype)
    pos = axis_positions(ev, nbr, r)
    acc = np.zeros(n, dtype)
    rows = np.arange(n)
    for a in range(d1):
        for b in range(d1):
            lo, hi, sgn = (a, b, -1) if a < b else (b, a, 1)
            s = sgn * ((pos > lo) & (pos <= hi)).astype(np.int64)          # [n, d+1]; all zero when a == b
            # the admissible c: s has both a zero and, when a != b, a -1 (a < b) or a +1 (a > b) among its entries
            for c in range(-r + (a < b), r + 1 - (a > b)):
                t = c + s
                alive = np.all(np.abs(t) <= r, axis=1)
                x = ev[:, a].copy()
                prod = np.ones(n, dtype)
                for j in range(d, -1, -1):
                    tj = t[:, j]
                    hop = alive & (tj != 0)
                    slot = np.where(tj < 0, tj + r, tj + r - 1)
                    nx = nbr[j, slot[hop], x[hop]] if r > 0 else x[hop]
                    x[hop] = nx
                    alive &= x >= 0
                    x[~alive] = 0
                    prod = np.where(alive, prod * taps[np.clip(tj + r, 0, 2 * r)], prod).astype(dtype)
                assert np.all(x[alive] == ev[alive, b]), "a surviving path ends at corner b"
                term = (ew[:, a] * ew[:, b]).astype(dtype) * prod
                acc = np.where(alive, acc + term, acc).astype(dtype)
    out = (acc / dtype(1.0 + 2.0 ** -d)).astype(dtype)
    if return_rank_check:
        # the nesting read from the table against the oracle's rank array: axis j_k is the coordinate of rank d + 1 - k
        want = np.where(rank == 0, 0, d1 - rank) if r > 0 else np.zeros_like(pos)
        return out, bool(np.array_equal(pos, want))
    return out
