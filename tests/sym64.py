"""TEST HELPER: the transposed and the symmetrised lattice operator in float64, on top of tests/lattice64.Lattice64.

    Kt64 = S B'_0 ... B'_d S^T / (1 + 2^-d)     B'_j: axis j with the taps mirrored (slot nid takes the coefficient
                                                of -nid) on the forward operator's structure, the axes in reverse order
    Ks64 = (K64 + Kt64) / 2

Kt64 is the construction the GPU uses (reversed axes, mirrored taps), NOT the transposed matrix: tests/test_sym64.py checks
on the CPU that the two agree, which is the identity the feature rests on (the neighbour table of a plain build is
symmetric).  Checker only: the product and the GPU path never import it.
"""
import copy

import numpy as np
import scipy.sparse as sp

from oracle import oracle
from tests.lattice64 import Lattice64

SYM_TAPS = np.array([0.5, 1.0, 0.5], np.float32)
LOPSIDED = {1: np.array([0.2, 0.85, 0.4], np.float32),
            2: np.array([0.1, 0.3, 0.85, 0.5, 0.2], np.float32)}


def taps_of(order, lopsided):
    """Taps of length 2 order + 1: the issue's two kinds where it names them ([0.5, 1, 0.5]; [0.2, 0.85, 0.4] and
    [0.1, 0.3, 0.85, 0.5, 0.2]), a Gaussian profile (times a ramp when lopsided) at the other orders."""
    if order == 1 and not lopsided:
        return SYM_TAPS.copy()
    if lopsided and order in LOPSIDED:
        return LOPSIDED[order].copy()
    j = np.arange(-order, order + 1)
    c = np.exp(-0.5 * (j * 0.7) ** 2)
    if lopsided:
        c = c * (1.0 + 0.35 * j / max(order, 1)) * 0.85
    return c.astype(np.float32)


def transposed64(ref, coeffs, fwd=None):
    """Kt64 as a Lattice64 (matrix / apply_staged / terms64 all follow its blurs): the structure of the forward operator
    `fwd` -- the same S, the same neighbour table -- with every axis blur rebuilt from mirrored taps (slot nid takes the
    coefficient of -nid) and the axes in reverse order.

    Not Lattice64(ref, coeffs[::-1]): the embedding's scale factors come from the fp32 variance of the taps, a sum that
    rounds differently once the taps are reversed, so that lattice is another lattice by an fp32 ulp of every coordinate
    (3.8e-7 between the two matrices at d = 1 with [0.2, 0.85, 0.4]); the GPU mirrors the taps on ONE build."""
    ref32 = np.ascontiguousarray(ref, np.float32)
    c32 = np.ascontiguousarray(np.asarray(coeffs, np.float32).reshape(-1))
    fwd = fwd if fwd is not None else Lattice64(ref32, c32)
    r, m, d = c32.size // 2, fwd.m, fwd.d
    oracle.set_exact_mode(False)
    try:
        lat = oracle.Lattice(ref32, c32)            # deterministic: the vertex numbering of `fwd`
    finally:
        oracle.set_exact_mode(True)
    assert int(lat.m) == m
    nbr = lat.neighbors() if r > 0 else np.empty((d + 1, 0, m), np.int32)
    lat.close()
    c = c32.astype(np.float64)
    nids = [t for t in range(-r, r + 1) if t != 0]
    ident = np.arange(m, dtype=np.int64)
    blurs = []
    for j in range(d + 1):
        rr, cc, vv = [ident], [ident], [np.full(m, c[r])]
        for s, nid in enumerate(nids):
            ids = nbr[j, s].astype(np.int64)
            ok = ids >= 0
            rr.append(ident[ok]); cc.append(ids[ok]); vv.append(np.full(int(ok.sum()), c[r - nid]))
        B = sp.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(m, m))
        B.sum_duplicates()
        blurs.append(B)
    kt = copy.copy(fwd)
    kt.blurs = blurs[::-1]
    kt._K = None
    return kt


class Sym64:
    """K64, Kt64 and Ks64 of one lattice."""

    def __init__(self, ref, coeffs):
        self.k = Lattice64(ref, coeffs)
        self.kt = transposed64(ref, coeffs, fwd=self.k)
        self.n, self.d, self.m = self.k.n, self.k.d, self.k.m

    def matrix(self):
        return 0.5 * (self.k.matrix() + self.kt.matrix())

    def apply_staged(self, v):
        return 0.5 * (self.k.apply_staged(v) + self.kt.apply_staged(v))

    def terms64(self, v):
        """The mean of the forward and the reverse terms: what an entry of Ks64 v sums."""
        return 0.5 * (self.k.terms64(v) + self.kt.terms64(v))
