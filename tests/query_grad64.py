"""TEST HELPER: the derivative of the query operator with respect to the query positions, in float64 -- the yardstick of
plx_slice_at_dots / plx_locate_pullback, query_grad.slice_at_backward, LatticeSliceAt and PredictionCache.predict_query_grad.

Inside the simplex of a query the barycentric weights are affine in the position: w_r(x) for r = 0..d with

    sum_r w_r P_r = el(x),   sum_r w_r = 1,                                    (*)

P_r the integer corner keys (d + 1 coordinates that sum to zero; tests/query64.Query64.qkeys holds the first d) and
el(x) = E x the elevated position, E[i, j] = s_j ([j >= i] - (j + 1) [i = j + 1]) with s = oracle.scale_factors.  The
Jacobian J[q, r, j] = d w_r / d x_j is derived two ways:

  geometric    differentiate (*): sum_r J_r P_r = E, sum_r J_r = 0, that is sum_{r >= 1} J_r (P_r - P_0) = E; the last key
               coordinate is minus the sum of the others, so the first d coordinates are a square system per query.  No
               rank enters.
  closed form  the pull-back the device uses.  With rk the rank permutation (read off the keys: corner r adds r to the
               coordinates of rank <= d - r and r - (d + 1) to the others, so rk_i = d - #{r >= 1: P_r[i] - P_0[i] = r}),
                   e_i  = (t_{d - rk_i} - t_{(d + 1 - rk_i) mod (d + 1)}) / (d + 1)
                   gx_j = s_j (sum_{i <= j} e_i - (j + 1) e_{j+1})
               maps t (a derivative with respect to the weights) to the position; J[:, r, :] is the image of the r-th unit t.

tests/test_query_grad64.py pins the two against each other and against central differences of Query64.apply64.

Checker only: the product and the GPU path never import it.
"""
import numpy as np

from oracle import oracle
from tests.query64 import Query64

U24 = 2.0 ** -24


def elevation_matrix(d, coeffs):
    """E [d+1, d] float64 with el = E x, from the oracle's fp32 scale factors."""
    s = oracle.scale_factors(d, coeffs).astype(np.float64)
    E = np.zeros((d + 1, d))
    for j in range(d):
        E[:j + 1, j] = s[j]
        E[j + 1, j] = -(j + 1) * s[j]
    return E, s


def full_keys(ref):
    """P [nq, d+1, d+1] int64: every corner key of every query with its last coordinate."""
    k = ref.qkeys.astype(np.int64)
    return np.concatenate([k, -k.sum(-1, keepdims=True)], -1)


def ranks(ref):
    """rk [nq, d+1]: the rank permutation of every query, from its corner keys alone."""
    P, d = full_keys(ref), ref.d
    hits = sum((P[:, r, :] - P[:, 0, :] == r).astype(np.int64) for r in range(1, d + 1)) if d >= 1 else 0
    rk = d - hits
    assert np.array_equal(np.sort(rk, -1), np.broadcast_to(np.arange(d + 1), rk.shape)), "the ranks are a permutation"
    return rk


def pullback64(rk, s, t):
    """The closed form: t [nq, d+1] -> gx [nq, d], float64."""
    d = len(s)
    d1 = d + 1
    t = np.asarray(t, np.float64)
    k = rk                                                      # u[k] = t[d - k] - t[(d + 1 - k) mod (d + 1)]
    e = (np.take_along_axis(t, d - k, 1) - np.take_along_axis(t, (d1 - k) % d1, 1)) / d1
    return s * (np.cumsum(e, 1)[:, :d] - np.arange(1, d1) * e[:, 1:])


def pullback_terms(rk, s, t_abs):
    """M [nq, d]: the size of the terms of pullback64 at |t| = t_abs -- s_j (sum_{i <= j} |e|_i + (j + 1) |e|_{j+1}) with
    |e|_i = (|t|_{d - rk_i} + |t|_{(d + 1 - rk_i) mod (d + 1)}) / (d + 1)."""
    d = len(s)
    d1 = d + 1
    t_abs = np.abs(np.asarray(t_abs, np.float64))
    e = (np.take_along_axis(t_abs, d - rk, 1) + np.take_along_axis(t_abs, (d1 - rk) % d1, 1)) / d1
    return s * (np.cumsum(e, 1)[:, :d] + np.arange(1, d1) * e[:, 1:])


def _differences(ref):
    """(D^T [nq, d, d], P_0 [nq, d]): the first d coordinates of P_r - P_0 for r = 1..d, transposed, and of P_0.  The
    differences are integers between -d and d wherever the cloud lies, so the solves below do not lose digits to the size of
    the keys (the last coordinate is minus the sum of the others and adds no equation)."""
    P, d = full_keys(ref).astype(np.float64), ref.d
    return np.swapaxes(P[:, 1:, :d] - P[:, :1, :d], 1, 2), P[:, 0, :d]


def weights64(ref, E, Q):
    """The weights (*) gives for the float64 positions Q in the simplices of `ref`: [nq, d+1] -- what the fp32 weights of
    the reference round.  sum_{r >= 1} w_r (P_r - P_0) = el - P_0, w_0 = 1 - sum_{r >= 1} w_r."""
    Dt, P0 = _differences(ref)
    rest = np.linalg.solve(Dt, (np.asarray(Q, np.float64) @ E[:ref.d].T - P0)[..., None])[..., 0]
    return np.concatenate([1.0 - rest.sum(1, keepdims=True), rest], 1)


class QueryGrad64:
    """The Jacobians of the queries of a Query64 `ref` (its taps: `coeffs`).

    J_geo, J     [nq, d+1, d]: d w_r / d x_j, the geometric solve and the closed form
    rk           [nq, d+1]"""

    def __init__(self, ref, coeffs):
        self.ref, self.d, self.nq = ref, ref.d, ref.nq
        d = self.d
        self.E, self.s = elevation_matrix(d, coeffs)
        Dt, _ = _differences(ref)                               # sum_{r >= 1} J_r (P_r - P_0) = E, J_0 = -sum_{r >= 1} J_r
        rest = np.linalg.solve(Dt, np.broadcast_to(self.E[:d], (ref.nq, d, d)))
        self.J_geo = np.concatenate([-rest.sum(1, keepdims=True), rest], 1)
        self.rk = ranks(ref)
        eye = np.eye(d + 1)
        self.J = np.stack([pullback64(self.rk, self.s, np.broadcast_to(eye[r], (ref.nq, d + 1))) for r in range(d + 1)], 1)

    def corner_rows(self, values, id_of=None):
        """values[vid] [nq, d+1, vd] float64 with the rows of absent corners zero; id_of: as Query64.slice_matrix."""
        ref = self.ref
        ids = np.arange(ref.m) if id_of is None else np.asarray(id_of, np.int64)
        v = np.asarray(values, np.float64)
        rows = np.where(ref.found[..., None], v[ids[np.where(ref.found, ref.vid, 0)]], 0.0)
        return rows

    def dots64(self, values, g, id_of=None):
        """(t, T) [nq, d+1]: t_r = <g, values_r> / denom at the corners found, 0 at the absent ones, and the size of its
        terms T_r = <|g|, |values_r|> / denom."""
        rows = self.corner_rows(values, id_of)
        g = np.asarray(g, np.float64)
        return (np.einsum("qc,qrc->qr", g, rows) / self.ref.denom,
                np.einsum("qc,qrc->qr", np.abs(g), np.abs(rows)) / self.ref.denom)

    def pull(self, t):
        return pullback64(self.rk, self.s, t)

    def terms(self, t_abs):
        return pullback_terms(self.rk, self.s, t_abs)

    def grad64(self, values, g, id_of=None):
        """d <g, slice_at(values)> / d x [nq, d] in float64 through the geometric Jacobian."""
        t, _ = self.dots64(values, g, id_of)
        return np.einsum("qr,qrj->qj", t, self.J_geo)

    def jacobian_apply(self, values, id_of=None):
        """d out[q, c] / d x_j [nq, vd, d]: J^T values / denom."""
        return np.einsum("qrc,qrj->qcj", self.corner_rows(values, id_of), self.J_geo) / self.ref.denom


def shifted(X, Q, coeffs, h, lattice):
    """For every axis j the queries moved by +h and -h along it, as float32 (plus [d][nq, d], minus [d][nq, d]), their
    Query64s, and kept [nq, d]: whether x + h e_j and x - h e_j have the d + 1 corner keys of x, in the same order -- the
    pairs on which the operator is linear between the two points."""
    Q = np.ascontiguousarray(Q, np.float32)
    base = Query64(X, Q, coeffs, lattice=lattice)
    nq, d = Q.shape
    kept = np.zeros((nq, d), bool)
    plus, minus = [], []
    for j in range(d):
        Qp, Qm = Q.copy(), Q.copy()
        Qp[:, j] = Q[:, j] + np.float32(h)
        Qm[:, j] = Q[:, j] - np.float32(h)
        rp, rm = Query64(X, Qp, coeffs, lattice=lattice), Query64(X, Qm, coeffs, lattice=lattice)
        kept[:, j] = (rp.qkeys == base.qkeys).all((1, 2)) & (rm.qkeys == base.qkeys).all((1, 2))
        plus.append((Qp, rp))
        minus.append((Qm, rm))
    return base, plus, minus, kept


def weight_error(ref, E, Q):
    """max |w32 - w64| / 2^-24 over the queries of `ref` at the positions Q: how far, in units of the fp32 roundoff of a
    number below 1, the reference's own fp32 weights are from the weights float64 gives in the same simplices."""
    return float(np.abs(ref.weight.astype(np.float64) - weights64(ref, E, Q)).max() / U24)


def end_to_end_bar(G, t64, T, d, vd, eps):
    """The bar of slice_at_backward [nq, d] (tests/test_query_grad_gpu.py): the pull-back's (d + 6) eps on the terms of the
    dots, themselves off by (vd + 3) eps T, plus that error pulled back."""
    return eps * ((d + 6) * G.terms(np.abs(t64) + (vd + 3) * eps * T) + (vd + 3) * G.terms(T))


def reference_error(G, t64, T, d, vd):
    """What grad64 itself may be off by: twice the distance between the two derivations of the Jacobian on these queries,
    and the roundings of its two float64 sums."""
    return (2 * np.einsum("qr,qrj->qj", np.abs(t64), np.abs(G.J_geo - G.J))
            + 2.0 ** -52 * np.einsum("qr,qrj->qj", (d + 1) * np.abs(t64) + vd * T, np.abs(G.J_geo)))


def weight_error_cap(s, Q):
    """An a-priori cap on weight_error, from the positions Q [nq, d] and the scale factors s alone (u = 2^-24, first order,
    one per cent added for the higher orders).  The embedding forms el by the recurrence el_d = -d p_{d-1} s_{d-1},
    el_i = (el_{i+1} - i p_{i-1} s_{i-1}) + (i + 2) p_i s_i, el_0 = el_1 + 2 p_0 s_0: every leaf product is rounded twice and
    then once per addition it passes, two additions per step, so a leaf of el_i meets at most 2 (d - i) + 4 <= 2 d + 4
    roundings and |d el_i| <= (2 d + 4) u A, A the sum of the sizes of all leaves.  sd_i = ((el_i - gr_i) scale) adds three
    roundings (the difference, the rounded 1 / (d + 1), the product) on a number of size at most 1:
    |d sd| <= (2 d + 4) u A / (d + 1) + 3 u.  A weight is a difference of two sd (one rounding, size at most 1), the zeroth
    weight sd_d + (1 + (0 - sd_0)) two roundings on sizes at most 2: |d w| <= 2 |d sd| + 4 u.  In units of u:
        c <= 2 (2 d + 4) A / (d + 1) + 10."""
    d = len(s)
    a = np.abs(np.asarray(Q, np.float64)) * s                                   # |p_j| s_j
    k = np.arange(1, d)
    A = d * a[:, d - 1] + 2 * a[:, 0] + (k * a[:, :d - 1] + (k + 2) * a[:, 1:]).sum(1)
    return float(1.01 * (2 * (2 * d + 4) * A.max() / (d + 1) + 10))
