"""TEST HELPER: the lattice operator sliced at points that are not the build's, in float64 -- the yardstick of
Lattice.locate / slice_at / apply_at and of PredictionCache's query route.

    K_q(Q, X) = S_Q B_d ... B_0 S_X^T / (1 + 2^-d)

S_Q holds a query's barycentric weights on those of its d + 1 simplex corners that are vertices of X's lattice; an absent
corner contributes nothing.  Everything comes from the CPU oracle, unchanged, with its exact mode off (as
tests/lattice64.Lattice64 builds it): one oracle lattice on X gives X's vertex keys in X's numbering; one on the stacked
[Q; X] gives, in its rows of Q, the key (through its own keys) and the fp32 weight of every corner of every query -- the
embedding of a point depends on the point alone -- and a dict over X's keys maps those keys to X's ids, or to -1.  The blurs
are Lattice64(X)'s.

Checker only: the product and the GPU path never import it.
"""
import numpy as np
import scipy.sparse as sp

from oracle import oracle
from tests.lattice64 import Lattice64


def _structure(ref, coeffs):
    """(keys [m, d] int16, entry_vertex [n, d+1], entry_weight [n, d+1] float32) of the oracle lattice on `ref`, copied out
    before the lattice is closed."""
    oracle.set_exact_mode(False)
    try:
        lat = oracle.Lattice(np.ascontiguousarray(ref, np.float32), coeffs)
    finally:
        oracle.set_exact_mode(True)
    try:
        return (np.array(lat.keys, np.int16, copy=True), np.array(lat.entry_vertex, np.int64, copy=True),
                np.array(lat.entry_weight, np.float32, copy=True))
    finally:
        lat.close()


def _key_bytes(keys):
    keys = np.ascontiguousarray(keys, np.int16)
    return [row.tobytes() for row in keys]


class Query64:
    """K_q(Q, X) for the positions X [n, d], the queries Q [nq, d] and the taps `coeffs`.

    vid      [nq, d+1] int64: the id, in X's oracle numbering, of every corner of every query, -1 where absent
    weight   [nq, d+1] float32: the barycentric weights (all of them, found or not)
    qkeys    [nq, d+1, d] int16: the key of every corner
    xkeys    [m, d] int16: X's vertex keys in X's oracle numbering
    mass32   [nq] float32: the sequential float32 sum, in corner order, of the weights of the corners found
    lattice  Lattice64(X, coeffs) (pass one already built to share it)"""

    def __init__(self, X, Q, coeffs, lattice=None):
        X = np.ascontiguousarray(X, np.float32)
        Q = np.ascontiguousarray(Q, np.float32)
        coeffs = np.ascontiguousarray(np.asarray(coeffs, np.float32).reshape(-1))
        self.lattice = lattice if lattice is not None else Lattice64(X, coeffs)
        L = self.lattice
        self.n, self.d, self.m, self.nq = L.n, L.d, L.m, Q.shape[0]
        d, nq = self.d, self.nq
        self.xkeys, _, _ = _structure(X, coeffs)
        assert self.xkeys.shape == (self.m, d)
        skeys, sev, sew = _structure(np.concatenate([Q, X], 0), coeffs)
        limit = 32767 - 2 * (d + 1)
        assert np.abs(skeys.astype(np.int64)).max() < limit and np.abs(self.xkeys.astype(np.int64)).max() < limit, \
            "a reference key left the range the device accepts"
        self.qkeys = skeys[sev[:nq]]                                    # [nq, d+1, d]
        self.weight = sew[:nq].copy()
        ids = {k: i for i, k in enumerate(_key_bytes(self.xkeys))}
        assert len(ids) == self.m, "X's vertex keys are distinct"
        self.vid = np.array([ids.get(k, -1) for k in _key_bytes(self.qkeys.reshape(-1, d))], np.int64).reshape(nq, d + 1)
        self.found = self.vid >= 0
        mass = np.zeros(nq, np.float32)
        for r in range(d + 1):                                          # the sequential fp32 sum, corner by corner
            mass = np.where(self.found[:, r], (mass + self.weight[:, r]).astype(np.float32), mass)
        self.mass32 = mass.astype(np.float32)
        self.S_Q = self.slice_matrix(np.arange(self.m))
        self.denom = L.denom

    @property
    def found_share(self):
        return float(self.found.mean())

    def slice_matrix(self, id_of):
        """S_Q [nq, m] (scipy CSR, float64) with X's oracle id v named id_of[v]: the identity for the oracle's own
        numbering, or the device's numbering of the same keys."""
        q, r = np.nonzero(self.found)
        cols = np.asarray(id_of, np.int64)[self.vid[q, r]]
        S = sp.csr_matrix((self.weight[q, r].astype(np.float64), (q, cols)), shape=(self.nq, self.m))
        S.sum_duplicates()
        return S

    def blurred64(self, v):
        """B_d ... B_0 S_X^T v [m, vd] in float64, X's oracle numbering."""
        L = self.lattice
        vals = L.S.T @ np.asarray(v, np.float64)
        for B in L.blurs:
            vals = B @ vals
        return vals

    def apply64(self, v):
        """K_q(Q, X) v for v [n, vd], float64."""
        return (self.S_Q @ self.blurred64(v)) / self.denom

    def terms64(self, v):
        """|S_Q| |B_d| ... |B_0| |S_X^T| |v| / denom: the size of the terms every entry of apply64(v) sums."""
        L = self.lattice
        vals = abs(L.S.T) @ np.abs(np.asarray(v, np.float64))
        for B in L.blurs:
            vals = abs(B) @ vals
        return (abs(self.S_Q) @ vals) / self.denom


def device_ids(xkeys, device_keys):
    """id_of [m]: the device's id of the vertex the oracle numbers v, from the two key arrays (the same set of keys)."""
    dev = {k: i for i, k in enumerate(_key_bytes(device_keys))}
    assert len(dev) == len(device_keys) == len(xkeys), "the device's keys are distinct and as many as the oracle's"
    return np.array([dev[k] for k in _key_bytes(xkeys)], np.int64)
