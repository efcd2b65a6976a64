"""longdouble references, the derived bars, the kernel-family table and the case list for the float64 exact kernel MVM
(plx_exact_f64.hip).  Plain numpy on the CPU: tests/test_exact_f64_host.py checks these helpers without a GPU,
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
import os
import re
import zlib

import numpy as np

from tests import exact64 as x64
from tests.exact64 import Case, DATA, KINDS, PROFILES  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "simplex_gp_amd", "csrc", "plx_exact_f64.hip")

LD = np.longdouble
U = 2.0 ** -53
DBL_MIN = float(np.finfo(np.float64).tiny)
TILE = 64                                            # kEx64TileJ
THREADS = 256                                        # kEx64Threads
SPLIT_J = 512                                        # kEx64SplitJ
MAX_SPLITS = 1024                                    # kEx64MaxSplits
WORK_CAP_BYTES = 16 << 20
DPS = (4, 8, 12, 16, 20, 24, 32)                     # the double ladders (the fp32 ones are kept)
TCS = (1, 4, 8, 16)
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


# ---- which kernel a call runs: ex64_dp / ex64_tc of plx_exact_f64.hip, restated -----------------------------------------
def ex_dp(d):
    for dp in DPS[:-1]:
        if d <= dp:
            return dp
    return DPS[-1]


def ex_tc(t):
    for tc in TCS[:-1]:
        if t <= tc:
            return tc
    return TCS[-1]


def family(kind, profile, d, t, splits):
    """(kind, profile, DP, TC, "direct" | "slabs"); splits is what plx_exact_splits_f64 returns for the call."""
    assert kind in KINDS and profile in PROFILES and splits >= 1
    return (kind, profile, ex_dp(d), ex_tc(t), "slabs" if splits > 1 else "direct")


FAMILIES = [(kind, p, dp, tc) for kind in KINDS for p in PROFILES for dp in DPS for tc in TCS]      # the 224 instantiations
# where the slab path must be reached as well: the slab stride is n1 t in the forward (every TC) and n1 d in the gradient
SLAB_FAMILIES = [("mvm", "TC", tc) for tc in TCS] + [("grad", "DP", dp) for dp in DPS]


def missing_coverage(reached):
    """What a set of family() results leaves out: instantiations of FAMILIES never run, and (kind, profile, axis, value)
    of SLAB_FAMILIES, per profile, never run on the slab path."""
    reached = set(reached)
    missing = sorted(set(FAMILIES) - {f[:4] for f in reached})
    slabs = [f for f in reached if f[4] == "slabs"]
    for kind, axis, value in SLAB_FAMILIES:
        for p in PROFILES:
            if not any(f[0] == kind and f[1] == p and f[2 if axis == "DP" else 3] == value for f in slabs):
                missing.append((kind, p, axis, value, "slabs"))
    return missing


def bar(kind, d, t, n2, splits):
    """The derived bound on |got - want| / T of one call (module docstring)."""
    dp, tc = ex_dp(d), ex_tc(t)
    chunk = -(-n2 // splits)
    tiles = -(-chunk // TILE)
    if kind == "mvm":
        return (TILE + dp + C_MVM + tiles + splits) * U
    return (TILE + dp + C_MVM + tc + 2 + tiles * -(-t // tc) + splits) * U


def parse_source(path=SOURCE):
    """What plx_exact_f64.hip holds: the template values its two dispatch switches launch, its ex64_dp / ex64_tc rules as
    ([(bound, value) ...], default), and the constants the case list is built around."""
    text = re.sub(r"//[^\n]*", "", open(path).read())
    found = {}
    for key, callee in (("dp", r"ex64_dispatch_tc<PROF,\s*"), ("tc", r"ex64_launch<PROF,\s*DP,\s*")):
        values = set()
        for m in re.finditer(r"(?:case\s+(\d+)|default)\s*:\s*%s(\d+)>" % callee, text):
            assert m.group(1) is None or m.group(1) == m.group(2), m.group(0)
            values.add(int(m.group(2)))
        found[key] = values
    for key, fn, arg in (("dp_rule", "ex64_dp", "d"), ("tc_rule", "ex64_tc", "t")):
        body = re.search(r"static int %s\(int %s\)\s*\{(.*?)\n\}" % (fn, arg), text, re.S).group(1)
        steps = [(int(a), int(b)) for a, b in re.findall(r"if \(%s <= (\d+)\) return (\d+);" % arg, body)]
        found[key] = (steps, int(re.search(r"\n\s*return (\d+);\s*$", body).group(1)))
    for key, name in (("tile", "kEx64TileJ"), ("threads", "kEx64Threads"), ("split_j", "kEx64SplitJ"),
                      ("max_splits", "kEx64MaxSplits")):
        found[key] = int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    return found


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
D_ENDS = {4: (1, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 20: (17, 20), 24: (21, 24), 32: (25, 32)}
T_EDGES = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33)       # both ends of every TC, and one, two and three column blocks
N1_EDGES = (1, 255, 256, 257)                      # one row; the 256-row workgroup with a dead lane, full, and one row over
N2_EDGES = (65, 1, 150, 63, 64)                    # the 64-row LDS tile: one row over, one row, three tiles, below, full
N2_STARTS = (0, 1, 2, 4)                           # rotations of N2_EDGES whose first two entries include more than one tile
T_RAGGED = (1, 3, 7, 19)                           # one t per TC, none a multiple of it (19: two column blocks)
# The named split shapes (n1, n2, d, t, splits), derived for the double workspace (slabs of doubles under 16 MiB = 2^21
# doubles; a slice covers at least 512 j; at most 1024 slices and 524288 slab rows):
# (a) two slices, neither a multiple of the 64-row tile, two row blocks: n2 // 512 = 2 slices of 750 = 11 * 64 + 46 rows
SPLIT_RAGGED = (257, 1500)
# (b) the maximum split count with the last slice empty: n2 // 512 = 1024 slices of ceil(524799 / 1024) = 513 rows, and
#     1023 * 513 = 524799 = n2; the gradient's slabs (1024 * 8 * 3 doubles) fill the workspace to the last double
SPLIT_EMPTY = (8, 524799, 3, 1, 1024)
# (c) a split count set by the 16 MiB cap: 2^21 doubles / 64 columns = 32768 slab rows = 127 slices of 257 rows (128 do
#     not fit), where n2 // 512 = 136 would be allowed
SPLIT_CAP = (257, 70001, 3, 64, 127)
CAP_ROWS = (0, 1, 255, 256)                        # the rows of (c) judged against longdouble: both workgroups, the dead-lane edge


def _cases():
    cases = []
    for ki, kind in enumerate(KINDS):
        for pi, profile in enumerate(PROFILES):
            for di, dp in enumerate(DPS):
                group = f"{kind}-{profile}-dp{dp}"
                rot = ki + pi + di
                idx = 0         # n1 turns with idx, the data kind with idx + idx // 4: the 20 cases hold all 16 (n1, data) pairs
                for t in T_EDGES:
                    for d in D_ENDS[dp]:
                        cases.append(Case(group, kind, profile, d, t, N1_EDGES[(idx + rot) % 4],
                                          N2_EDGES[(idx + N2_STARTS[rot % 4]) % 5], DATA[(idx + idx // 4 + rot) % 4]))
                        idx += 1
                # (a) the ragged split: every TC in the forward, one per (profile, DP) in the gradient (TC in rotation)
                for ti, t in enumerate(T_RAGGED if kind == "mvm" else (T_RAGGED[rot % 4],)):
                    cases.append(Case(group, kind, profile, D_ENDS[dp][(ti + rot) % 2], t, *SPLIT_RAGGED, DATA[(ti + rot) % 3]))
    n1, n2, d, t, _ = SPLIT_EMPTY
    cases += [Case(f"split-empty-{kind}", kind, p, d, t, n1, n2, "range") for kind, p in
              (("mvm", "rbf"), ("mvm", "matern32"), ("grad", "matern12"), ("grad", "matern52"))]
    return cases


CASES = _cases()
n1_, n2_, d_, t_, _s = SPLIT_CAP
CAP_CASES = [Case("split-cap-mvm", "mvm", "matern52", d_, t_, n1_, n2_, "range"),
             Case("split-cap-grad", "grad", "rbf", d_, t_, n1_, n2_, "range")]
GROUPS = list(dict.fromkeys(c.group for c in CASES))
EDGE_GROUPS = [g for g in GROUPS if not g.startswith("split-")]      # one per (kind, profile, DP)
