"""longdouble references, the derived bars, the kernel-family table and the case list for the float64 exact kernel MVM
(plx_exact_kernels.h with T = double).  Plain numpy on the CPU: tests/test_exact_f64_host.py checks these helpers without a GPU,
tests/test_exact_f64_gpu.py holds the kernels against them.

The measure is exact64's: every output entry is compared with its reference in units of a yardstick T, the sum of the
absolute values of the terms the entry adds up, each weighted by 1 + a_ij (a_ij the magnitude of the exponential's
argument: a relative rounding of the argument is an absolute error a in the exponent); where T is 0 the entry must be
exactly 0.  The references are evaluated in np.longdouble (64-bit mantissa on x86) from the doubles the kernel receives,
and those doubles are NOT fp32-representable (make_data), so anything rounded through float is off by ~2^-24 of T, nine
orders of magnitude above the bars.

The bars are derived, never measured (bar()).  u = 2^-53.  An entry is off, to first order, by at most
    (TILE + DP + C + tiles * blocks + splits) u T
    TILE            the tile's sequential sum: at most 64 additions (the FMAs into the tile accumulator), each rounding
                    at most u of a partial sum that T bounds
    DP + C          the roundings of one term, relative to its weight (1 + a): the differences (one rounding each, 2 u of
                    a squared term) and the DP FMAs of d2 give d2 to (DP + 2) u; sqrt (<= 1 ulp), the Matern constant (a
                    rounded literal) and its product give s = const * r to ((DP + 2) / 2 + 4) u, which the exponential
                    turns into a ((DP + 2) / 2 + 4) u; exp itself is good to 1 ulp = 2 u; the Matern polynomial
                    1 + s + (5 / 3) d2 adds at most (DP + 6) u and its product with exp one more: (DP + 9) u (1 + a) for
                    matern52, the longest; RBF needs (DP + 2) u (1 + a).  C_MVM = 12 holds every profile with 3 to spare
                    for the second-order terms.  The gradient's 2 k' has the same count or less (matern12: one division
                    in place of the polynomial), and a term carries three more factors: the dot g_i . v_j, a sequential
                    sum of TC FMAs (TC u of sum_c |g_ic| |v_jc|), its product with 2 k', and the rounded difference:
                    C_GRAD = 12 + TC + 2
    tiles * blocks  one addition per tile of the slice to the running sum (the gradient keeps one running sum over all
                    column blocks of t: tiles * ceil(t / TC) additions; the forward's running sum is per block)
    splits          one addition per slab
The reference's own error (2^-64 per operation, 2^-11 u) and the comparison in longdouble add nothing visible."""
import zlib

import numpy as np

from tests import exact64 as x64
# what does not depend on the scalar type is exact64's: the ladders and the family table, the edges of every size but n2
# (the tile differs), two of the three named split shapes, and the one parser of the one source
from tests.exact64 import (Case, DATA, KINDS, PROFILES, DPS, TCS, ex_dp, ex_tc, family, FAMILIES, SLAB_FAMILIES,  # noqa: F401
                           missing_coverage, parse_source, D_ENDS, T_EDGES, N1_EDGES, N2_STARTS, T_RAGGED, SPLIT_RAGGED,
                           SPLIT_EMPTY)

LD = np.longdouble
U = 2.0 ** -53
DBL_MIN = float(np.finfo(np.float64).tiny)
TILE = 64                                            # ExScalar<double>::kTileJ
THREADS = 256                                        # kExThreads
SPLIT_J = 512                                        # kExSplitJ
MAX_SPLITS = 1024                                    # kExMaxSplits
WORK_CAP_BYTES = 16 << 20
C_MVM = 12
BLOCK_PAIRS = 1 << 20                                # longdouble differences held at a time: n1 * block * d
PERTURB = 2.0 ** -30


# ---- references ------------------------------------------------------------------------------------------------------
def ld(a):
    return np.asarray(a, LD)


def profile_ld(d2, profile):
    """(k, 2 k', a) of a longdouble array of squared distances; 2 k' of matern12 is 0 at r = 0."""
    if profile == "rbf":
        e = np.exp(-d2)
        return e, LD(-2) * e, d2
    r = np.sqrt(d2)
    if profile == "matern12":
        e = np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            return e, np.where(r > 0, -e / r, LD(0)), r
    if profile == "matern32":
        s = np.sqrt(LD(3)) * r
        e = np.exp(-s)
        return (LD(1) + s) * e, LD(-3) * e, s
    assert profile == "matern52", profile
    s = np.sqrt(LD(5)) * r
    e = np.exp(-s)
    return (LD(1) + s + (LD(5) / LD(3)) * d2) * e, (LD(-5) / LD(3)) * (LD(1) + s) * e, s


def _blocks(n1, n2, d):
    step = max(1, BLOCK_PAIRS // max(1, n1 * d))
    return [(j, min(n2, j + step)) for j in range(0, n2, step)]


def mvm_ld(x1, x2, v, profile):
    """(K v, T) in longdouble: out[i][c] = sum_j k(d2_ij) v[j][c], T[i][c] = sum_j k(d2_ij) |v[j][c]| (1 + a_ij)."""
    x1, x2, v = ld(x1), ld(x2), ld(v)
    n1, n2, t = x1.shape[0], x2.shape[0], v.shape[1]
    out, T = np.zeros((n1, t), LD), np.zeros((n1, t), LD)
    with np.errstate(under="ignore"):
        for j0, j1 in _blocks(n1, n2, x1.shape[1]):
            diff = x1[:, None, :] - x2[None, j0:j1, :]
            k, _, a = profile_ld((diff * diff).sum(-1), profile)
            out += k @ v[j0:j1]
            T += (k * (LD(1) + a)) @ np.abs(v[j0:j1])
    return out, T


def grad_ld(x1, x2, g, v, profile):
    """(grad_x1, T) in longdouble: grad[i][k] = sum_j 2 k'(d2_ij) (x1_ik - x2_jk) (g_i . v_j) and
    T[i][k] = sum_j |2 k'(d2_ij)| |x1_ik - x2_jk| (sum_c |g_ic| |v_jc|) (1 + a_ij)."""
    x1, x2, g, v = ld(x1), ld(x2), ld(g), ld(v)
    n1, n2, d = x1.shape[0], x2.shape[0], x1.shape[1]
    out, T = np.zeros((n1, d), LD), np.zeros((n1, d), LD)
    with np.errstate(under="ignore"):
        for j0, j1 in _blocks(n1, n2, d):
            diff = x1[:, None, :] - x2[None, j0:j1, :]
            _, dk2, a = profile_ld((diff * diff).sum(-1), profile)
            vj = v[j0:j1]
            out += np.einsum("ij,ijk->ik", dk2 * (g @ vj.T), diff)
            T += np.einsum("ij,ijk->ik", np.abs(dk2) * (np.abs(g) @ np.abs(vj).T) * (LD(1) + a), np.abs(diff))
    return out, T


def mvm_floor(n2, v):
    """The absolute error every forward entry is allowed before the ratio counts: a term below the double normal range
    keeps fewer bits or is flushed, n2 terms of at most DBL_MIN max|v| each."""
    return n2 * DBL_MIN * float(np.abs(v).max())


def grad_floor(x1, x2, g, v):
    """The analogous product for the gradient: n2 DBL_MIN max|x1_ik - x2_jk| max_i (sum_c |g_ic|) max|v|."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    span = max(float((x1.max(0) - x2.min(0)).max()), float((x2.max(0) - x1.min(0)).max()), 0.0)
    return np.shape(x2)[0] * DBL_MIN * span * float(np.abs(g).sum(1).max()) * float(np.abs(v).max())


def entry_ratio(got, want, T, floor=0.0):
    """max over the entries of |got - want| / T, the difference taken in longdouble; an entry whose T is 0 must be
    exactly 0 (else inf) and no entry may be NaN or inf.  floor: an absolute error allowed before the ratio counts."""
    got, want, T = np.broadcast_arrays(ld(got), ld(want), ld(T))
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.maximum(np.abs(got - want) - LD(floor), LD(0))
    zero = T == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float((err[~zero] / T[~zero]).max()) if np.any(~zero) else 0.0


def bar(kind, d, t, n2, splits):
    """The derived bound on |got - want| / T of one call (module docstring)."""
    dp, tc = ex_dp(d), ex_tc(t)
    chunk = -(-n2 // splits)
    tiles = -(-chunk // TILE)
    if kind == "mvm":
        return (TILE + dp + C_MVM + tiles + splits) * U
    return (TILE + dp + C_MVM + tc + 2 + tiles * -(-t // tc) + splits) * U


# ---- data ------------------------------------------------------------------------------------------------------------
def _perturb(a, g):
    """every value moved by a relative 2^-31 .. 2^-30 (either sign): a double no float holds; zeros stay zeros"""
    rel = (0.5 + 0.5 * g.random(a.shape)) * np.where(g.random(a.shape) < 0.5, -1.0, 1.0)
    return a.astype(np.float64) * (1.0 + PERTURB * rel)


def make_data(case):
    """The doubles of a case: exact64.make_data's arrays (its four kinds: cloud, shift by 30, coincident, far), every value
    perturbed off the fp32 grid.  Coincident rows stay coincident (r = 0 off the diagonal)."""
    base = x64.make_data(case)
    g = np.random.default_rng(zlib.crc32(repr(("f64",) + tuple(case)).encode()))
    out = {k: _perturb(base[k], g) for k in ("x1", "x2", "v", "g")}
    if case.data == "coincident":
        m1, m2 = (case.n1 + 1) // 2, (case.n2 + 1) // 2
        out["x2"][:m2] = out["x2"][0]
        out["x1"][:m1] = out["x2"][0]
    return out


def off_fp32_grid(a):
    """True where every non-zero value of the double array a differs from its rounding to fp32."""
    a = np.asarray(a, np.float64)
    return bool(np.all((a.astype(np.float32).astype(np.float64) != a) | (a == 0)))


# ---- cases -----------------------------------------------------------------------------------------------------------
N2_EDGES = (65, 1, 150, 63, 64)                    # the 64-row LDS tile: one row over, one row, three tiles, below, full
# The named split shapes (n1, n2, d, t, splits), derived for the double workspace (slabs of doubles under 16 MiB = 2^21
# doubles; a slice covers at least 512 j; at most 1024 slices and 524288 slab rows).  exact64's SPLIT_RAGGED and
# SPLIT_EMPTY hold here as well:
# (a) two slices, neither a multiple of the 64-row tile, two row blocks: n2 // 512 = 2 slices of 750 = 11 * 64 + 46 rows
# (b) the maximum split count with the last slice empty: n2 // 512 = 1024 slices of ceil(524799 / 1024) = 513 rows, and
#     1023 * 513 = 524799 = n2; the gradient's slabs (1024 * 8 * 3 doubles) fill the workspace to the last double
# (c) a split count set by the 16 MiB cap: 2^21 doubles / 64 columns = 32768 slab rows = 127 slices of 257 rows (128 do
#     not fit), where n2 // 512 = 136 would be allowed
SPLIT_CAP = (257, 70001, 3, 64, 127)
CAP_ROWS = (0, 1, 255, 256)                        # the rows of (c) judged against longdouble: both workgroups, the dead-lane edge

CASES = x64._cases(N2_EDGES, "split-empty-{kind}")
CAP_CASES = x64.cap_cases(SPLIT_CAP)
GROUPS = list(dict.fromkeys(c.group for c in CASES))
EDGE_GROUPS = [g for g in GROUPS if not g.startswith("split-")]      # one per (kind, profile, DP)
