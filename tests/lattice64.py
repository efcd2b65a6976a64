"""TEST HELPER: the lattice operator in float64, the yardstick of the position gradient.

The structure comes from the CPU oracle with its exact mode off (oracle.Lattice): the duplicate-free lattice that the HIP
build reproduces bit for bit, found without HIP.  From it the linear operator is assembled with scipy.sparse in float64:

    S[p, entry_vertex[p, i]] = entry_weight[p, i]                                  (n x m, duplicates summed)
    B_j = c[r] I + sum_s c[nid_s + r] N_{j,s}       j = 0..d, nid_s = -r..-1, 1..r (plxo_neighbors' slot order)
    K64 = S B_d ... B_0 S^T / (1 + 2^-d)

i.e. the oracle's splat / blur / slice with every sum carried in float64 (the weights themselves are the build's fp32
values).  terms64 is the size of the terms each entry of K64 v sums, the yardstick of a per-entry error.  backward64 is the position gradient of out = K(x) src (py:113-123) on top of it, stack and contraction in
float64, together with the size of the terms that the gradient is a difference of.

Checker only: the product and the GPU path never import it.
"""
import numpy as np
import scipy.sparse as sp

from oracle import oracle


class Lattice64:
    """K64 for the positions `ref` [n, d] and the taps `coeffs` (odd length)."""

    def __init__(self, ref, coeffs):
        ref = np.ascontiguousarray(ref, np.float32)
        coeffs = np.ascontiguousarray(np.asarray(coeffs, np.float32).reshape(-1))
        oracle.set_exact_mode(False)
        try:
            lat = oracle.Lattice(ref, coeffs)
        finally:
            oracle.set_exact_mode(True)
        self.n, self.d = ref.shape
        self.m = int(lat.m)
        self.coeffs = coeffs.astype(np.float64)
        n, d, m = self.n, self.d, self.m
        r = coeffs.size // 2
        ev = lat.entry_vertex.astype(np.int64)
        ew = lat.entry_weight.astype(np.float64)
        rows = np.repeat(np.arange(n, dtype=np.int64), d + 1)
        self.S = sp.csr_matrix((ew.reshape(-1), (rows, ev.reshape(-1))), shape=(n, m))
        self.S.sum_duplicates()
        nbr = lat.neighbors() if r > 0 else np.empty((d + 1, 0, m), np.int32)
        lat.close()
        self.blurs = []
        nids = [t for t in range(-r, r + 1) if t != 0]
        ident = np.arange(m, dtype=np.int64)
        for j in range(d + 1):
            rr, cc, vv = [ident], [ident], [np.full(m, self.coeffs[r])]
            for s, nid in enumerate(nids):
                ids = nbr[j, s].astype(np.int64)
                ok = ids >= 0                        # an absent neighbour contributes nothing
                rr.append(ident[ok]); cc.append(ids[ok]); vv.append(np.full(int(ok.sum()), self.coeffs[nid + r]))
            B = sp.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(m, m))
            B.sum_duplicates()
            self.blurs.append(B)
        self.denom = 1.0 + 2.0 ** -d
        self._K = None

    def matrix(self):
        """The dense n x n float64 matrix of K64 (formed once: the blurs run over the sparse columns of S^T)."""
        if self._K is None:
            G = self.S.T.tocsr()
            for B in self.blurs:
                G = (B @ G).tocsr()
            K = (self.S @ G)
            self._K = (K.toarray() if sp.issparse(K) else np.asarray(K)) / self.denom
        return self._K

    def apply(self, v):
        """K64 v for v [n, vd] (any float dtype; the product is float64)."""
        v = np.asarray(v, np.float64)
        return self.matrix() @ v

    def apply_staged(self, v):
        """The same product as splat / blur / slice on the vertex values (no n x n matrix; any n)."""
        vals = self.S.T @ np.asarray(v, np.float64)
        for B in self.blurs:
            vals = B @ vals
        return (self.S @ vals) / self.denom

    def terms64(self, v):
        """|S| |B_d| ... |B_0| |S^T| |v| / denom: row i bounds the sum of the magnitudes of every product that entry i of
        K v adds up (so |K64 v| <= terms64(v) elementwise, with equality for non-negative v and taps).  An fp32 kernel that
        carries each sum in fp32 stays within a small multiple of its rounding unit times this, row by row."""
        vals = abs(self.S.T) @ np.abs(np.asarray(v, np.float64))
        for B in self.blurs:
            vals = abs(B) @ vals
        return (abs(self.S) @ vals) / self.denom


def stack64(g, src, x):
    """[g | g (x) x | src | src (x) x] in float64 (py:113-119): n x 2L(1+d), l-major within each product block."""
    g, src, x = (np.asarray(a, np.float64) for a in (g, src, x))
    n, L = g.shape
    d = x.shape[1]
    gx = (g[:, :, None] * x[:, None, :]).reshape(n, L * d)
    sx = (src[:, :, None] * x[:, None, :]).reshape(n, L * d)
    return np.concatenate([g, gx, src, sx], axis=1)


def contract64(g, src, x, filtered):
    """(grad_x, grad_src, T) from the filtered stack, all in float64 (py:122-123):
        grad_x[p, k] = -2 sum_l ( s_l x_k wg_l - s_l wgx_lk + g_l x_k ws_l - g_l wsx_lk )
        T[p, k]      =  2 sum_l ( |s_l x_k wg_l| + |s_l wgx_lk| + |g_l x_k ws_l| + |g_l wsx_lk| )
    T is what the gradient is a difference of: where the true gradient vanishes (isolated points: wgx = x wg exactly)
    an fp32 result can only be judged against it."""
    g, src, x, f = (np.asarray(a, np.float64) for a in (g, src, x, filtered))
    n, L = g.shape
    d = x.shape[1]
    wg, wgx, ws, wsx = np.split(f, [L, L + L * d, 2 * L + L * d], axis=1)
    wgx = wgx.reshape(n, L, d)
    wsx = wsx.reshape(n, L, d)
    s3, g3, x3 = src[:, :, None], g[:, :, None], x[:, None, :]
    t1 = s3 * x3 * wg[:, :, None]
    t2 = s3 * wgx
    t3 = g3 * x3 * ws[:, :, None]
    t4 = g3 * wsx
    grad_x = -2.0 * (t1 - t2 + t3 - t4).sum(1)
    T = 2.0 * (np.abs(t1) + np.abs(t2) + np.abs(t3) + np.abs(t4)).sum(1)
    return grad_x, wg.copy(), T


def backward64(g, src, x, deriv_coeffs, lattice=None):
    """Position gradient of out = K(x) src with the upstream gradient g, on the lattice of x built with the DERIVATIVE
    taps (py:113-123): returns (grad_x [n, d], grad_src [n, L] = wg, T [n, d]), all float64.  `lattice`: a Lattice64 of
    (x, deriv_coeffs) already built (reused across calls)."""
    lat = lattice if lattice is not None else Lattice64(x, deriv_coeffs)
    return contract64(g, src, x, lat.apply(stack64(g, src, x)))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def entry_ratio(got, want, T):
    """max_i |got - want|_i / T_i over every entry: the per-entry error in units of the size of the terms it sums.  Where
    T_i = 0 (no term reaches the entry: an isolated vertex of a zero input) got_i must be exactly 0, else the ratio is inf."""
    got, want, T = (np.asarray(a, np.float64) for a in (got, want, T))
    err = np.abs(got - want)
    zero = T == 0
    if np.any(err[zero] != 0) or not np.all(np.isfinite(got)):
        return float("inf")
    return float((err[~zero] / T[~zero]).max()) if np.any(~zero) else 0.0


def grad_x_ratios(got, want, T):
    """(||got - want|| / ||T||, rel-L2 or None): the second only where the gradient does not vanish
    (||want|| >= 0.1 ||T||), where a relative bar means something."""
    got, want, T = (np.asarray(a, np.float64) for a in (got, want, T))
    tn = float(np.linalg.norm(T))
    terms = float(np.linalg.norm(got - want)) / max(tn, 1e-300)
    rel = rel_l2(got, want) if np.linalg.norm(want) >= 0.1 * tn else None
    return terms, rel


# ---- point clouds where lattice kernels go wrong ------------------------------------------------------------------------
CLOUDS = ("gauss0.3", "gauss1", "gauss3", "simplex", "isolated")


def cloud(kind, n, d, seed=0, coeffs=None):
    """float32 positions [n, d]:
    gauss<s>  Gaussian of scale s;
    simplex   every point inside one simplex (long vertex rows: n points on each of d+1 vertices);
    isolated  points so far apart that no two share a vertex or a blur neighbour: the true position gradient is 0
              (their lattice coordinates stay within int16 keys: the spacing is set by the taps' scale factors);
    dup       a Gaussian cloud of n // 3 distinct points, each repeated;
    grid      points on a coarse grid of half-integer coordinates (ties: many points on the same spot, others on the
              boundaries between simplices)."""
    rng = np.random.default_rng(seed)
    if kind.startswith("gauss"):
        return (rng.standard_normal((n, d)) * float(kind[5:])).astype(np.float32)
    if kind == "simplex":
        c = coeffs if coeffs is not None else np.array([0.5, 1.0, 0.5], np.float32)
        for _ in range(100):                  # a centre far enough from every face that the whole cloud stays inside
            x = (rng.standard_normal(d) * 0.5 + 1e-5 * rng.standard_normal((n, d))).astype(np.float32)
            oracle.set_exact_mode(False)
            try:
                lat = oracle.Lattice(x, c)
            finally:
                oracle.set_exact_mode(True)
            m = lat.m
            lat.close()
            if m == d + 1:
                return x
        raise RuntimeError(f"no one-simplex cloud found at d = {d}")
    if kind == "isolated":
        # a grid over the first min(d, 3) axes, 12 blur steps of the lattice apart (a step moves a key coordinate by d)
        sf = oracle.scale_factors(d, coeffs if coeffs is not None else np.array([0.5, 1.0, 0.5], np.float32))
        a = min(d, 3)
        k = int(np.ceil(n ** (1.0 / a) - 1e-9))
        idx = np.arange(n)
        x = rng.standard_normal((n, d)) * 0.3
        for j in range(a):
            x[:, j] += (idx // k ** j % k - (k - 1) / 2) * (12.0 * d / float(sf[j]))
        return x[rng.permutation(n)].astype(np.float32)
    if kind == "dup":
        base = rng.standard_normal((max(1, n // 3), d))
        return base[rng.integers(0, base.shape[0], n)].astype(np.float32)
    if kind == "grid":
        return (rng.integers(-3, 4, (n, d)) * 0.5).astype(np.float32)
    raise ValueError(kind)
