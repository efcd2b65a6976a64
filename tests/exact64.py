"""float64 references, error measures, the kernel-family table and the case list for the exact kernel MVM
(plx_exact_kernels.h with T = float).  Plain numpy on the CPU: tests/test_exact64.py checks these helpers without a GPU,
tests/test_exact_fp64.py holds the kernels against them.

The measure follows lattice64 / solver64.entry_ratio: every output entry is compared with its float64 value in units
of a yardstick T, the sum of the absolute values of the terms that entry adds up; where T is 0 the entry must be exactly
0.  Here every term carries a factor (1 + a_ij), a_ij the magnitude of the exponential's argument (d2 for rbf; r,
sqrt(3) r, sqrt(5) r for the Materns): the kernel evaluates __expf of an fp32 argument, a relative rounding of the
argument is an absolute error a in the exponent, so a far pair is legitimately less accurate relative to its own size
than a near one.  The references take the SAME fp32 values the kernel receives and evaluate the formulas in the header
of plx_exact_kernels.h by direct differences in float64."""
import collections
import os
import re
import zlib

import numpy as np

from tests.solver64 import FLT_MIN, entry_ratio, f64  # noqa: F401  (entry_ratio is this module's measure too)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "simplex_gp_amd", "csrc", "plx_exact_kernels.h")

PROFILES = ("rbf", "matern12", "matern32", "matern52")          # index = PLX_PROFILE_*
DPS = (4, 8, 12, 16, 20, 24, 32)
TCS = (1, 4, 8, 16)
KINDS = ("mvm", "grad")
KERNELS = {"mvm": "exact_mvm_kernel", "grad": "exact_grad_kernel"}
SLAB_KERNEL = "exact_sum_slabs_kernel"                              # runs in every "slabs" call
BLOCK_PAIRS = 1 << 21                                               # differences held at a time: n1 * block * d


# ---- references ------------------------------------------------------------------------------------------------------
def profile64(d2, profile):
    """(k, 2 k', a) of a float64 array of squared distances; 2 k' of matern12 is 0 at r = 0 (the header's convention)."""
    if profile == "rbf":
        e = np.exp(-d2)
        return e, -2.0 * e, d2
    r = np.sqrt(d2)
    if profile == "matern12":
        e = np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            return e, np.where(r > 0, -e / r, 0.0), r
    if profile == "matern32":
        s = np.sqrt(3.0) * r
        e = np.exp(-s)
        return (1.0 + s) * e, -3.0 * e, s
    assert profile == "matern52", profile
    s = np.sqrt(5.0) * r
    e = np.exp(-s)
    return (1.0 + s + (5.0 / 3.0) * d2) * e, (-5.0 / 3.0) * (1.0 + s) * e, s


def _blocks(n1, n2, d):
    step = max(1, BLOCK_PAIRS // max(1, n1 * d))
    return [(j, min(n2, j + step)) for j in range(0, n2, step)]


def mvm64(x1, x2, v, profile):
    """(K v, T): out[i][c] = sum_j k(d2_ij) v[j][c] and T[i][c] = sum_j k(d2_ij) |v[j][c]| (1 + a_ij)."""
    x1, x2 = f64(x1), f64(x2)
    n1, n2, t = x1.shape[0], x2.shape[0], np.shape(v)[1]
    out, T = np.zeros((n1, t)), np.zeros((n1, t))
    for j0, j1 in _blocks(n1, n2, x1.shape[1]):
        diff = x1[:, None, :] - x2[None, j0:j1, :]
        k, _, a = profile64((diff * diff).sum(-1), profile)
        vj = f64(v[j0:j1])
        out += k @ vj
        T += (k * (1.0 + a)) @ np.abs(vj)
    return out, T


def grad64(x1, x2, g, v, profile):
    """(grad_x1, T): grad[i][k] = sum_j 2 k'(d2_ij) (x1_ik - x2_jk) (g_i . v_j) and
    T[i][k] = sum_j |2 k'(d2_ij)| |x1_ik - x2_jk| (sum_c |g_ic| |v_jc|) (1 + a_ij)."""
    x1, x2, g = f64(x1), f64(x2), f64(g)
    n1, n2, d = x1.shape[0], x2.shape[0], x1.shape[1]
    out, T = np.zeros((n1, d)), np.zeros((n1, d))
    for j0, j1 in _blocks(n1, n2, d):
        diff = x1[:, None, :] - x2[None, j0:j1, :]
        _, dk2, a = profile64((diff * diff).sum(-1), profile)
        vj = f64(v[j0:j1])
        out += np.einsum("ij,ijk->ik", dk2 * (g @ vj.T), diff)
        T += np.einsum("ij,ijk->ik", np.abs(dk2) * (np.abs(g) @ np.abs(vj).T) * (1.0 + a), np.abs(diff))
    return out, T


def mvm_floor(n2, v):
    """The absolute error every forward entry is allowed before the ratio counts: the GPU flushes a term below the fp32
    normal range, n2 terms of at most FLT_MIN max|v| each."""
    return n2 * FLT_MIN * float(np.abs(f64(v)).max())


def grad_floor(x1, x2, g, v):
    """The analogous product for the gradient: n2 FLT_MIN max|x1_ik - x2_jk| max_i (sum_c |g_ic|) max|v|."""
    x1, x2 = f64(x1), f64(x2)
    span = max(float((x1.max(0) - x2.min(0)).max()), float((x2.max(0) - x1.min(0)).max()), 0.0)
    return np.shape(x2)[0] * FLT_MIN * span * float(np.abs(f64(g)).sum(1).max()) * float(np.abs(f64(v)).max())


# ---- which kernel a call runs: ex_dp / ex_tc of plx_exact_kernels.h, restated (for both scalar types) ----------------------
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
    """(kind, profile, DP, TC, "direct" | "slabs"); splits is what plx_exact_splits returns for the call."""
    assert kind in KINDS and profile in PROFILES and splits >= 1
    return (kind, profile, ex_dp(d), ex_tc(t), "slabs" if splits > 1 else "direct")


FAMILIES = [(kind, p, dp, tc) for kind in KINDS for p in PROFILES for dp in DPS for tc in TCS]      # the 224 instantiations
# where the slab path must be reached as well: the slab stride is n1 t in the forward (every TC) and n1 d in the gradient
SLAB_FAMILIES = [("mvm", "TC", tc) for tc in TCS] + [("grad", "DP", dp) for dp in DPS]


def missing_coverage(reached):
    """What a set of family() results leaves out: instantiations of FAMILIES never run, and (kind, profile, axis, value)
    of SLAB_FAMILIES, per profile, never run on the slab path.  Both acceptance tests (case list, GPU run) assert it empty."""
    reached = set(reached)
    missing = sorted(set(FAMILIES) - {f[:4] for f in reached})
    slabs = [f for f in reached if f[4] == "slabs"]
    for kind, axis, value in SLAB_FAMILIES:
        for p in PROFILES:
            if not any(f[0] == kind and f[1] == p and f[2 if axis == "DP" else 3] == value for f in slabs):
                missing.append((kind, p, axis, value, "slabs"))
    return missing


def parse_source(path=SOURCE):
    """What plx_exact_kernels.h holds, for both scalar types (tests/exact_f64.py reads it too): {"kernels": the __global__ kernel
    names, "dp" / "tc": the template values the switches of ex_dispatch_dp / ex_dispatch_tc launch (case N must launch
    <N>), "dp_rule" / "tc_rule": ex_dp / ex_tc as ([(bound, value) ...], default), "profiles": the PLX_PROFILE_* names that
    have a Profile<> specialisation, "dispatched": those ex_run dispatches, "threads" / "split_j" / "max_splits": the
    constants of those names, and "tile": {scalar type: rows of the LDS tile}}."""
    text = re.sub(r"//[^\n]*", "", open(path).read())
    found = {"kernels": set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\(", text))}
    for key, callee in (("dp", r"ex_dispatch_tc<T,\s*PROF,\s*"), ("tc", r"ex_launch<T,\s*PROF,\s*DP,\s*")):
        values = set()
        for m in re.finditer(r"(?:case\s+(\d+)|default)\s*:\s*%s(\d+)>" % callee, text):
            assert m.group(1) is None or m.group(1) == m.group(2), m.group(0)
            values.add(int(m.group(2)))
        found[key] = values
    for key, fn, arg in (("dp_rule", "ex_dp", "d"), ("tc_rule", "ex_tc", "t")):
        body = re.search(r"static int %s\(int %s\)\s*\{(.*?)\n\}" % (fn, arg), text, re.S).group(1)
        steps = [(int(a), int(b)) for a, b in re.findall(r"if \(%s <= (\d+)\) return (\d+);" % arg, body)]
        found[key] = (steps, int(re.search(r"\n\s*return (\d+);\s*$", body).group(1)))
    found["profiles"] = set(re.findall(r"template\s*<typename T>\s*struct\s+Profile<T,\s*PLX_PROFILE_(\w+)>", text))
    found["dispatched"] = set(re.findall(r"ex_dispatch_dp<T,\s*PLX_PROFILE_(\w+)>", text))
    for key, name in (("threads", "kExThreads"), ("split_j", "kExSplitJ"), ("max_splits", "kExMaxSplits")):
        found[key] = int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    tiles = re.findall(r"struct ExScalar<(\w+)>\s*\{[^}]*?constexpr int kTileJ = (\d+);", text)
    found["tile"] = {scalar: int(rows) for scalar, rows in tiles}
    assert len(found["tile"]) == len(tiles)
    return found


# ---- data ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "group kind profile d t n1 n2 data")
DATA = ("range", "shift", "coincident", "far")
FAR = 200.0              # displacement of the far row: every profile's k and k' lie below 1e-80 there, far below FLT_MIN
SHIFT = 30.0


def _rng(*seed):
    return np.random.default_rng(zlib.crc32(repr(seed).encode()))


def _cloud(n, d, g):
    """rows of three spreads in rotation: pair distances from about 0.1 to about 4, the range where the profiles matter"""
    scale = np.array([0.3, 1.0, 2.5])[np.arange(n) % 3] / np.sqrt(2.0 * d)
    return (g.standard_normal((n, d)) * scale[:, None]).astype(np.float32)


def _columns(n, t, g, shift):
    """[n][t] values; the column kinds rotate through random, all zero, one sign and cancelling (neighbouring rows of
    nearly opposite values)"""
    a = g.standard_normal((n, t)).astype(np.float32)
    for c in range(t):
        kind = (c + shift) % 4
        if kind == 1:
            a[:, c] = 0
        elif kind == 2:
            a[:, c] = np.abs(a[:, c]) + np.float32(0.25)
        elif kind == 3:
            u = (g.random(n) + 0.5).astype(np.float32)
            sign = np.where(np.arange(n) % 2 == 0, 1.0, -(1.0 - 2e-6)).astype(np.float32)
            a[:, c] = np.repeat(u[::2], 2)[:n] * sign
    return a


def make_data(case):
    """The fp32 arrays of a case: x1 [n1][d], x2 [n2][d] (distinct arrays), v [n2][t], g [n1][t] (the gradient's)."""
    g = _rng(*case)
    x1, x2 = _cloud(case.n1, case.d, g), _cloud(case.n2, case.d, g)
    if case.data == "coincident":                   # r = 0 off the diagonal: half of each cloud sits on one point
        m1, m2 = (case.n1 + 1) // 2, (case.n2 + 1) // 2
        x2[:m2] = x2[0]
        x1[:m1] = x2[0]
    if case.data == "far":                          # one row whose every term lies below FLT_MIN
        x1[0, 0] += np.float32(FAR)
    if case.data == "shift":
        x1, x2 = x1 + np.float32(SHIFT), x2 + np.float32(SHIFT)
    return dict(x1=x1, x2=x2, v=_columns(case.n2, case.t, g, 0), g=_columns(case.n1, case.t, g, 2))


# ---- cases -----------------------------------------------------------------------------------------------------------
D_ENDS = {4: (1, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 20: (17, 20), 24: (21, 24), 32: (25, 32)}
T_EDGES = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33)       # both ends of every TC, and one, two and three column blocks
N1_EDGES = (1, 255, 256, 257)                      # one row; the 256-row workgroup with a dead lane, full, and one row over
N2_EDGES = (129, 1, 300, 127, 128)                 # the 128-row LDS tile: below, full, one row over, three tiles, one row
N2_STARTS = (0, 1, 2, 4)                           # rotations of N2_EDGES whose first two entries include more than one tile
T_RAGGED = (1, 3, 7, 19)                           # one t per TC, none a multiple of it (19: two column blocks)
# the named split shapes (n1, n2, d, t) and the split count each must have
SPLIT_RAGGED = (257, 1500)                         # (a) 2 slices of 750 rows: no multiple of the tile, two row blocks
SPLIT_EMPTY = (8, 524799, 3, 1, 1024)              # (b) 1024 slices of 513 rows, the last one empty
SPLIT_CAP = (257, 140001, 3, 64, 255)              # (c) n2 / 512 = 273 slices fit the row bound, the 16 MB cap allows 255


def _cases(n2_edges, empty_group):
    """The edge and ragged-split cases of every (kind, profile, DP) and the SPLIT_EMPTY ones, for a kernel whose n2 edges
    (around its LDS tile) are n2_edges; empty_group names the group of a SPLIT_EMPTY case ("{kind}" is filled in)."""
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
                                          n2_edges[(idx + N2_STARTS[rot % 4]) % 5], DATA[(idx + idx // 4 + rot) % 4]))
                        idx += 1
                # (a) the ragged split: every TC in the forward, one per (profile, DP) in the gradient (TC in rotation)
                for ti, t in enumerate(T_RAGGED if kind == "mvm" else (T_RAGGED[rot % 4],)):
                    cases.append(Case(group, kind, profile, D_ENDS[dp][(ti + rot) % 2], t, *SPLIT_RAGGED, DATA[(ti + rot) % 3]))
    n1, n2, d, t, _ = SPLIT_EMPTY
    cases += [Case(empty_group.format(kind=kind), kind, p, d, t, n1, n2, "range") for kind, p in
              (("mvm", "rbf"), ("mvm", "matern32"), ("grad", "matern12"), ("grad", "matern52"))]
    return cases


def cap_cases(split_cap):
    """The two cases of a SPLIT_CAP shape (n1, n2, d, t, splits)."""
    n1, n2, d, t, _ = split_cap
    return [Case("split-cap-mvm", "mvm", "matern52", d, t, n1, n2, "range"),
            Case("split-cap-grad", "grad", "rbf", d, t, n1, n2, "range")]


CASES = _cases(N2_EDGES, "split-empty") + cap_cases(SPLIT_CAP)
GROUPS = list(dict.fromkeys(c.group for c in CASES))
EDGE_GROUPS = [g for g in GROUPS if not g.startswith("split-")]      # one per (kind, profile, DP)
