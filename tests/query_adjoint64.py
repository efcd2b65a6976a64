"""TEST HELPER: the adjoint of the query operator in float64 -- the yardstick of query_adjoint.splat_at / slice_at_adjoint /
apply_at_t.

    S_Q^T g                                              the splat at the query points      (splat_at64)
    K_q^T g = S_X (B_0^T ... B_d^T (S_Q^T g)) / denom    the transposed query product       (apply_t64)

on top of tests/query64.Query64: the same S_Q, the same blurs, the same S_X.  The sums of splat_at64 are formed in
np.longdouble with np.add.at, one term after the other, so that the float64 bar of the device's splat is not spent on the
reference's own rounding; what the blurs and the slice add in float64 is inside apply_at_t's bar (its depth counts them).

Checker only: the product and the GPU path never import it.
"""
import numpy as np

# The inputs of the per-entry contract of tests/test_query_adjoint_gpu.py, as keys of tests/test_query_gpu.CASES, each with
# the five query sets of that file.  tests/test_query_adjoint64.py asserts their conditions from the reference alone.
SPLAT_CASES = [("gauss1", 1, 3, True, None), ("gauss1", 3, 1, True, None), ("dup", 8, 0, False, None),
               ("gauss1", 8, 2, False, None), ("gauss1", 18, 3, False, 300)]
SPLAT_SETS = ("train", "jit", "fresh", "far", "grid")
# every vertex touched, the longest sums (m = 3, cmax = 130): for depth, exempt from the untouched-vertex condition
DEPTH_CASE = ("simplex", 2, 0, False, None)
# (case, set) that find no corner at all beside every "far" set: second all-absent cases, the output is all zeros
ALL_ABSENT = {(("gauss1", 18, 3, False, 300), "fresh"), (("gauss1", 18, 3, False, 300), "grid")}
# (case, set) where c_v <= 1 throughout IS the point.  d = 18: the one-corner-per-vertex regime, every sum a single product
# that must come back with one rounding and no neighbour's term.  gauss1 at d = 8 with a fresh draw or the grid: one corner
# in a hundred is found, the plan is almost all absent keys and ptr almost constant.
SINGLE = {(("gauss1", 18, 3, False, 300), "train"), (("gauss1", 18, 3, False, 300), "jit"),
          (("gauss1", 8, 2, False, None), "fresh"), (("gauss1", 8, 2, False, None), "grid")}


class QueryAdjoint64:
    """The adjoint side of a Query64 `ref`.  `id_of` [m]: the name of X's oracle vertex v in the numbering the results are
    wanted in (default: the oracle's own).

    counts   [m] int64: the found corners of the queries at every vertex, c_v
    cmax     max(c_v)"""

    def __init__(self, ref, id_of=None):
        self.ref = ref
        self.id_of = np.arange(ref.m) if id_of is None else np.asarray(id_of, np.int64)
        self.q, r = np.nonzero(ref.found)                                 # the found corners, in (q, r) order
        self.v = self.id_of[ref.vid[self.q, r]]
        self.w = ref.weight[self.q, r].astype(np.longdouble)              # fp32 weights, exact in any wider format
        self.counts = np.bincount(self.v, minlength=ref.m).astype(np.int64)
        self.cmax = int(self.counts.max()) if self.counts.size else 0

    def _splat(self, g):
        g = np.asarray(g, np.float64)
        acc = np.zeros((self.ref.m, g.shape[1]), np.longdouble)
        np.add.at(acc, self.v, self.w[:, None] * g[self.q].astype(np.longdouble))
        return acc

    def splat_at64(self, g):
        """S_Q^T g [m, vd] for g [nq, vd]: longdouble sums, returned in longdouble."""
        return self._splat(g)

    def splat_terms64(self, g):
        """|S_Q|^T |g|: the size of the terms every entry of splat_at64(g) sums."""
        return self._splat(np.abs(np.asarray(g, np.float64)))

    def _chain_t(self, vals, absolute):
        """S_X (B_0^T ... B_d^T vals) / denom in float64, in the ORACLE's numbering (vals arrives in id_of's)."""
        L = self.ref.lattice
        vals = np.asarray(vals, np.float64)[self.id_of]                   # row v of the oracle's numbering
        for B in reversed(L.blurs):
            vals = (abs(B).T if absolute else B.T) @ vals
        return ((abs(L.S) if absolute else L.S) @ vals) / self.ref.denom

    def apply_t64(self, g):
        """K_q^T g [n, vd] in float64."""
        return self._chain_t(self.splat_at64(g), False)

    def terms_t64(self, g):
        """The same chain on absolute values: the size of the terms every entry of apply_t64(g) sums."""
        return self._chain_t(self.splat_terms64(g), True)
