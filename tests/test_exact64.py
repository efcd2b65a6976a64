"""tests/exact64.py itself, on the CPU: the float64 references of the exact kernel MVM against a naive double loop and a
finite difference, the error measure, the family table against plx_exact_kernels.h, and the acceptance test of the case list of
tests/test_exact_fp64.py (which instantiation and which path every case runs is a host-side fact: plx_exact_splits)."""
import math

import numpy as np
import pytest

from tests import exact64 as x64


def _k_naive(r2, profile):
    r = math.sqrt(r2)
    if profile == "rbf":
        return math.exp(-r2), -2 * math.exp(-r2), r2
    if profile == "matern12":
        return math.exp(-r), (-math.exp(-r) / r if r > 0 else 0.0), r
    if profile == "matern32":
        s = math.sqrt(3) * r
        return (1 + s) * math.exp(-s), -3 * math.exp(-s), s
    s = math.sqrt(5) * r
    return (1 + s + 5 * r2 / 3) * math.exp(-s), -5 / 3 * (1 + s) * math.exp(-s), s


def _tiny(seed, n1=5, n2=7, d=3, t=2):
    g = np.random.default_rng(seed)
    x1, x2 = g.standard_normal((n1, d)).astype(np.float32), g.standard_normal((n2, d)).astype(np.float32)
    x2[1] = x1[2]                                            # a pair at r = 0
    return x1, x2, g.standard_normal((n2, t)).astype(np.float32), g.standard_normal((n1, t)).astype(np.float32)


@pytest.mark.parametrize("profile", x64.PROFILES)
def test_references_against_a_double_loop(profile, monkeypatch):
    x1, x2, v, g = _tiny(1)
    n1, n2, d, t = 5, 7, 3, 2
    out, T = np.zeros((n1, t)), np.zeros((n1, t))
    gr, Tg = np.zeros((n1, d)), np.zeros((n1, d))
    for i in range(n1):
        for j in range(n2):
            diff = [float(x1[i, k]) - float(x2[j, k]) for k in range(d)]
            k, dk2, a = _k_naive(sum(e * e for e in diff), profile)
            dot = sum(float(g[i, c]) * float(v[j, c]) for c in range(t))
            adot = sum(abs(float(g[i, c]) * float(v[j, c])) for c in range(t))
            for c in range(t):
                out[i, c] += k * float(v[j, c])
                T[i, c] += k * abs(float(v[j, c])) * (1 + a)
            for q in range(d):
                gr[i, q] += dk2 * diff[q] * dot
                Tg[i, q] += abs(dk2) * abs(diff[q]) * adot * (1 + a)
    for block in (x64.BLOCK_PAIRS, 30):                      # 30: two rows of x2 at a time, the blocked path
        monkeypatch.setattr(x64, "BLOCK_PAIRS", block)
        got, gT = x64.mvm64(x1, x2, v, profile)
        assert np.allclose(got, out, rtol=1e-13, atol=0) and np.allclose(gT, T, rtol=1e-13, atol=0)
        got, gT = x64.grad64(x1, x2, g, v, profile)
        assert np.allclose(got, gr, rtol=1e-12, atol=1e-15) and np.allclose(gT, Tg, rtol=1e-13, atol=0)
        assert np.all(gT >= np.abs(got) * (1 - 1e-12)) and np.all(T >= np.abs(out) * (1 - 1e-12))


@pytest.mark.parametrize("profile", x64.PROFILES)
def test_grad64_is_the_derivative_of_mvm64(profile):
    """central finite difference of sum(g * mvm64) in float64; no pair at r = 0 (matern12 has a kink there)"""
    rng = np.random.default_rng(2)
    x1, x2 = rng.standard_normal((4, 3)), rng.standard_normal((6, 3))
    v, g = rng.standard_normal((6, 2)), rng.standard_normal((4, 2))
    got, _ = x64.grad64(x1, x2, g, v, profile)
    h = 1e-6
    for i in range(4):
        for k in range(3):
            e = np.zeros_like(x1)
            e[i, k] = h
            fd = ((x64.mvm64(x1 + e, x2, v, profile)[0] - x64.mvm64(x1 - e, x2, v, profile)[0]) * g).sum() / (2 * h)
            assert got[i, k] == pytest.approx(fd, rel=1e-6, abs=1e-9), (i, k)


def test_matern12_pair_at_r_zero_adds_nothing_and_zero_terms_demand_exact_zero():
    x = np.array([[1.0, 2.0]], np.float32)
    g = v = np.ones((1, 1), np.float32)
    for profile in x64.PROFILES:
        got, T = x64.grad64(x, x.copy(), g, v, profile)
        assert np.all(got == 0) and np.all(T == 0) and np.all(np.isfinite(got))
        assert x64.entry_ratio(np.zeros((1, 2)), got, T) == 0.0
        assert x64.entry_ratio(np.array([[0.0, 1e-30]]), got, T) == float("inf")
        assert x64.entry_ratio(np.array([[0.0, 1e-30]]), got, T, floor=1e-29) == 0.0
    out, T = x64.mvm64(x, x + 1, np.zeros((1, 3), np.float32), "rbf")            # an all-zero column: T = 0
    assert np.all(T == 0) and x64.entry_ratio(out, out, T) == 0.0
    assert x64.entry_ratio(out + 1e-40, out, T) == float("inf")
    assert x64.entry_ratio(np.array([np.nan]), np.array([1.0]), np.array([1.0])) == float("inf")
    assert x64.entry_ratio(np.array([1.5]), np.array([1.0]), np.array([2.0])) == 0.25


def test_floors_and_the_far_row():
    """the far row's terms all lie below FLT_MIN for every profile: its float64 value is within the floor of 0"""
    case = x64.Case("x", "grad", "matern12", 3, 2, 4, 9, "far")
    data = x64.make_data(case)
    assert x64.mvm_floor(9, data["v"]) == 9 * x64.FLT_MIN * float(np.abs(data["v"]).max())
    for profile in x64.PROFILES:
        out, T = x64.mvm64(data["x1"], data["x2"], data["v"], profile)
        assert np.all(np.abs(out[0]) < x64.FLT_MIN * 1e-40) and np.any(np.abs(out[1:]) > 1e-3)
        gr, _ = x64.grad64(data["x1"], data["x2"], data["g"], data["v"], profile)
        assert np.all(np.abs(gr[0]) < x64.FLT_MIN * 1e-40)
    assert x64.grad_floor(data["x1"], data["x2"], data["g"], data["v"]) > 9 * x64.FLT_MIN * 190


def test_data_of_a_case():
    for data in x64.DATA:
        case = x64.Case("x", "mvm", "rbf", 5, 6, 9, 12, data)
        a, b = x64.make_data(case), x64.make_data(case)
        assert all(a[k].dtype == np.float32 and np.array_equal(a[k], b[k]) for k in a)                # reproducible
        assert a["x1"].shape == (9, 5) and a["x2"].shape == (12, 5) and a["v"].shape == (12, 6) and a["g"].shape == (9, 6)
        assert np.all(a["v"][:, 1] == 0) and np.all(a["v"][:, 2] > 0) and np.all(a["g"][:, 3] == 0)
        assert abs(float(a["v"][:, 3].astype(np.float64).sum())) < 1e-4 * float(np.abs(a["v"][:, 3]).sum())     # cancelling
    co = x64.make_data(x64.Case("x", "grad", "matern12", 5, 6, 9, 12, "coincident"))
    assert np.array_equal(co["x1"][:5], co["x2"][:5]) and np.array_equal(co["x2"][0], co["x2"][5])
    assert float(x64.make_data(x64.Case("x", "mvm", "rbf", 5, 6, 9, 12, "shift"))["x2"].mean()) > 29


def test_exact_families_name_every_kernel_and_template_value():
    """FAMILIES is exactly profiles x DP x TC of the two templated kernels as plx_exact_kernels.h dispatches them, the slab kernel
    is the only other kernel, and ex_dp / ex_tc are restated correctly: a new value or profile fails here until exact64
    (and so a case) names it."""
    src = x64.parse_source()
    assert src["kernels"] == set(x64.KERNELS.values()) | {x64.SLAB_KERNEL}
    assert src["dp"] == set(x64.DPS) and src["tc"] == set(x64.TCS)
    tile = src["tile"]["float"]                                  # the fp32 tile is what N2_EDGES is built around
    assert tile == 128 and set(x64.N2_EDGES) == {1, tile - 1, tile, tile + 1, 300} and 300 > 2 * tile
    assert src["profiles"] == src["dispatched"] == {p.upper() for p in x64.PROFILES}
    assert len(x64.FAMILIES) == 224 == len(set(x64.FAMILIES))
    assert set(x64.FAMILIES) == {(k, p, dp, tc) for k in x64.KERNELS for p in x64.PROFILES for dp in src["dp"] for tc in src["tc"]}
    for (steps, default), mine, top in ((src["dp_rule"], x64.ex_dp, 32), (src["tc_rule"], x64.ex_tc, 100)):
        assert {v for _, v in steps} | {default} == ({*x64.DPS} if top == 32 else {*x64.TCS})
        for n in range(1, top + 1):
            assert mine(n) == next((v for bound, v in steps if n <= bound), default), n
    assert [x64.D_ENDS[dp] for dp in x64.DPS] == [(1, 4), (5, 8), (9, 12), (13, 16), (17, 20), (21, 24), (25, 32)]
    assert all(x64.ex_dp(lo) == x64.ex_dp(hi) == dp and (lo == 1 or x64.ex_dp(lo - 1) < dp) for dp, (lo, hi) in x64.D_ENDS.items())
    assert [x64.ex_tc(t) for t in x64.T_EDGES] == [1, 4, 4, 8, 8, 16, 16, 16, 16, 16]
    assert [x64.ex_tc(t) for t in x64.T_RAGGED] == list(x64.TCS) and all(t % tc for t, tc in zip(x64.T_RAGGED[1:], x64.TCS[1:]))


@pytest.fixture(scope="module")
def lib():
    from simplex_gp_amd import _native
    return _native.lib()


def _splits(lib, c):
    return lib.plx_exact_splits(c.n1, c.n2, c.d, c.t)


def test_case_list_reaches_every_instantiation_and_both_paths(lib):
    """Acceptance, without a GPU: the cases of tests/test_exact_fp64.py reach all 224 instantiations, the slab path at
    every TC of the forward and every DP of the gradient (for every profile), and the three named split shapes with the
    split counts they were chosen for."""
    reached = set()
    for c in x64.CASES:
        s = _splits(lib, c)
        assert s >= 1, c
        fam = x64.family(c.kind, c.profile, c.d, c.t, s)
        reached.add(fam)
    assert x64.missing_coverage(reached) == []
    assert x64.missing_coverage({f for f in reached if f[:4] != ("grad", "rbf", 12, 8)}) == [("grad", "rbf", 12, 8)]
    assert ("mvm", "rbf", "TC", 8, "slabs") in x64.missing_coverage({f for f in reached if f[:2] != ("mvm", "rbf") or f[3:] != (8, "slabs")})
    slabs = {f[:4] for f in reached if f[4] == "slabs"}
    assert {f for f in slabs if f[0] == "mvm"} == {f for f in x64.FAMILIES if f[0] == "mvm"}       # in fact: every forward one
    # every instantiation sees both ends of its d range or a padded t, more than one tile of x2 and a dead lane
    per = {}
    for c in x64.CASES:
        per.setdefault((c.kind, c.profile, x64.ex_dp(c.d), x64.ex_tc(c.t)), []).append(c)
    for fam, cs in per.items():
        assert any(c.n2 > 128 for c in cs) and any(c.n1 % 256 for c in cs), fam
        assert {c.d for c in cs} >= set(x64.D_ENDS[fam[2]]), fam
    assert len(x64.EDGE_GROUPS) == len(x64.KINDS) * len(x64.PROFILES) * len(x64.DPS)
    for group in x64.EDGE_GROUPS:
        cs = [c for c in x64.CASES if c.group == group]
        assert {c.n1 for c in cs} >= set(x64.N1_EDGES) and {c.n2 for c in cs} >= set(x64.N2_EDGES), group
        assert {c.t for c in cs} >= set(x64.T_EDGES) and {c.data for c in cs} == set(x64.DATA), group
        edge = [c for c in cs if (c.n1, c.n2) != x64.SPLIT_RAGGED]
        assert {(c.n1, c.data) for c in edge} == {(n1, data) for n1 in x64.N1_EDGES for data in x64.DATA}, group
        assert {(c.n1, c.n2) for c in edge} == {(n1, n2) for n1 in x64.N1_EDGES for n2 in x64.N2_EDGES}, group
        assert all(c.n1 <= 300 and c.n2 <= 1500 for c in cs)
    assert set(x64.GROUPS) - set(x64.EDGE_GROUPS) == {"split-empty", "split-cap-mvm", "split-cap-grad"}


def test_named_split_shapes_have_the_stated_split_counts(lib):
    n1, n2 = x64.SPLIT_RAGGED
    ragged = [c for c in x64.CASES if (c.n1, c.n2) == (n1, n2)]
    assert len(ragged) == 4 * 28 + 28 and all(_splits(lib, c) == 2 for c in ragged)
    assert -(-n2 // 2) == 750 and 750 % 128 and n1 > 256                                  # two ragged slices, two row blocks
    n1, n2, d, t, s = x64.SPLIT_EMPTY
    assert (n1, n2, d, t, s) == (8, 524799, 3, 1, 1024) and lib.plx_exact_splits(n1, n2, d, t) == s
    chunk = -(-n2 // s)
    assert chunk == 513 and (s - 1) * chunk == n2                                          # the last slice is empty
    assert lib.plx_exact_work_bytes(n1, n2, d, t) == 4 * s * n1 * d                        # the gradient's slabs fill it
    assert sum(1 for c in x64.CASES if c.group == "split-empty") == 4
    n1, n2, d, t, s = x64.SPLIT_CAP
    assert lib.plx_exact_splits(n1, n2, d, t) == s
    assert n2 // 512 > s and 2048 // 2 > s and n1 * (n2 // 512) <= 524288                  # neither n2 / 512, the chip nor the rows
    assert s == (1 << 22) // t // n1 and lib.plx_exact_work_bytes(n1, n2, d, t) == 16 << 20        # ... but the 16 MB cap
    assert 4 * s * n1 * t <= 16 << 20 < 4 * (s + 1) * n1 * t
    assert {c.kind for c in x64.CASES if c.group.startswith("split-cap")} == {"mvm", "grad"}
