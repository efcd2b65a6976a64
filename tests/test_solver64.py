"""CPU checks of tests/solver64.py: each helper gives ratio 0 for the float64 value itself, about one fp32 ulp for the
fp32-rounded value and far more for one flipped entry; the family table names every kernel and every dispatched
template value of the three solver sources."""
import numpy as np

from tests import solver64 as s64

ULP = 2.0 ** -23
BAD = 1e-3          # a flipped entry must show at least this far above an fp32 rounding


def _three(got64, T, flip):
    """(ratio of the fp64 value, of its fp32 rounding, of the rounding with entry `flip` negated)"""
    got32 = np.asarray(got64, np.float32)
    bad = got32.copy()
    bad.flat[flip] = -bad.flat[flip] if bad.flat[flip] != 0 else 1.0
    return s64.entry_ratio(got64, got64, T), s64.entry_ratio(got32, got64, T), s64.entry_ratio(bad, got64, T)


def _rng(seed):
    return np.random.default_rng(seed)


def test_entry_ratio_zero_terms_demand_exact_zero():
    assert s64.entry_ratio([0.0, 1.0], [0.0, 1.0], [0.0, 2.0]) == 0.0
    assert s64.entry_ratio([1e-30, 1.0], [0.0, 1.0], [0.0, 2.0]) == float("inf")
    assert s64.entry_ratio([np.nan, 1.0], [0.0, 1.0], [1.0, 2.0]) == float("inf")
    assert s64.entry_ratio(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))) == 0.0
    assert s64.entry_ratio([1.5], [1.0], [2.0]) == 0.25
    assert s64.rel_ratio([0.0], [0.0]) == 0.0 and s64.rel_ratio([1.0], [0.0]) == float("inf")


def test_coldot_and_colsum():
    g = _rng(0)
    a, b = g.standard_normal((1000, 7)).astype(np.float32), g.standard_normal((1000, 7)).astype(np.float32)
    a[:, 2] = 0
    want, T = s64.coldot64(a, b)
    assert np.allclose(want, (a.astype(np.float64) * b).sum(0)) and T[2] == 0 and np.all(T >= np.abs(want))
    z, r, bad = _three(want, T, 4)
    assert z == 0 and r <= ULP and bad > BAD
    want2, T2 = s64.colsum64(a)
    z, r, bad = _three(want2, T2, 0)
    assert z == 0 and r <= ULP and bad > BAD


def test_axpy_and_coefficients():
    g = _rng(1)
    y, x = g.standard_normal((50, 5)).astype(np.float32), g.standard_normal((50, 5)).astype(np.float32)
    a = g.standard_normal(5).astype(np.float32)
    want, T = s64.axpy64(y, a, x)
    z, r, bad = _three(want, T, 17)
    assert z == 0 and r <= ULP and bad > BAD
    rs, pap = np.array([2.0, 3.0, 0.5, 1.0], np.float32), np.array([4.0, -1.0, 0.0, 2.0], np.float32)
    al = s64.alpha64(rs, pap, np.array([1, 1, 1, 0], np.float32))
    assert al[0] == 0.5 and al[3] == 0 and np.isclose(al[1], 3e30) and np.isclose(al[2], 0.5e30)
    flag, decided = s64.active64(np.array([1, 1, 1, 0, 1, 1.0]), np.array([4.0, 1.0, 1.0, 9.0, 1.0, 0.0]),
                                 np.array([1.0, 1.0, 0.9995, 1.0, 0.0, 0.0]), 1.0)
    assert flag.tolist() == [1, 0, 1, 0, 1, 0] and decided.tolist() == [True, False, False, True, True, True]


def test_project_and_apply():
    g = _rng(2)
    kp, k, n, t = 32, 20, 300, 5
    L = np.zeros((kp, n), np.float32)
    L[:k] = g.standard_normal((k, n)) * 0.3
    R = g.standard_normal((n, t)).astype(np.float32)
    C = L[:k].astype(np.float64) @ L[:k].T + 0.4 * np.eye(k)
    cinv = np.eye(kp) / 0.4
    cinv[:k, :k] = np.linalg.inv(C)
    want, T = s64.project64(L, R, cinv)
    assert np.allclose(want[:k], np.linalg.solve(C, L[:k].astype(np.float64) @ R)) and np.all(T[k:] == 0) and np.all(want[k:] == 0)
    z, r, bad = _three(want, T, 3)
    assert z == 0 and r <= ULP and bad > BAD
    Td = np.zeros((kp, 16), np.float32)
    Td[:, :t] = want
    Z, TZ = s64.apply64(L, k, R, Td, (1.0, 2.5))
    assert np.allclose(Z, (R - L[:k].astype(np.float64).T @ Td[:k, :t]) * 2.5)
    z, r, bad = _three(Z, TZ, 11)
    assert z == 0 and r <= ULP and bad > BAD
    Z0, TZ0 = s64.apply64(L, 0, R, Td, (1.0, 2.5))
    assert np.array_equal(Z0, R.astype(np.float64) * 2.5) and np.array_equal(TZ0, np.abs(Z0))


def test_lanczos_step_is_the_three_term_recurrence_with_reorthogonalisation():
    g = _rng(3)
    n, i = 400, 5
    Q, _ = np.linalg.qr(g.standard_normal((n, i + 1)))
    Q = Q.T.astype(np.float32)
    w = g.standard_normal(n).astype(np.float32)
    ref = s64.lanczos_step64(Q, w, i)
    Qd = Q.astype(np.float64)
    proj = w - Qd.T @ (Qd @ w)
    assert np.allclose(ref["w"], proj, atol=1e-6) and np.isclose(ref["alpha"], Qd[i] @ w, atol=1e-6)
    assert np.isclose(ref["beta"], np.linalg.norm(proj), rtol=1e-6) and np.allclose(ref["q"] * ref["beta"], ref["w"])
    assert np.max(np.abs(Qd @ ref["q"])) < 1e-6
    z, r, bad = _three(ref["w"], ref["Tw"], 100)
    assert z == 0 and r <= ULP and bad > BAD
    assert s64.entry_ratio(np.float32(ref["alpha"]), ref["alpha"], ref["Talpha"]) <= ULP
    assert s64.entry_ratio(-ref["alpha"], ref["alpha"], ref["Talpha"]) > BAD
    first = s64.lanczos_step64(Q, w, 0)          # one basis row: both passes act on row 0
    assert np.isclose(first["alpha"], Qd[0] @ w, atol=1e-6)


def test_pchol64_is_the_pivoted_cholesky():
    g = _rng(4)
    n = 60
    x = g.standard_normal((n, 2))
    A = np.exp(-((x[:, None] - x[None]) ** 2).sum(-1)) * np.outer(1.01 ** -np.arange(n), 1.01 ** -np.arange(n))
    A = (A + 1e-3 * np.eye(n)).astype(np.float32)
    piv, cols, terms, d, gaps = s64.pchol64(A, np.diag(A), [], n, 0.0)
    assert sorted(piv) == list(range(n)) and np.allclose(cols.T @ cols, A, atol=1e-6) and np.all(d == 0)
    assert np.all(terms >= np.abs(cols) - 1e-12)
    # continued from a state it left: the same columns
    piv2, cols2, _, _, _ = s64.pchol64(A, s64.pchol64(A, np.diag(A), [], 7, 0.0)[3], cols[:7], 5, 0.0)
    assert piv2 == piv[7:12] and np.allclose(cols2, cols[7:12], atol=1e-12)
    z, r, bad = _three(cols[:12], terms[:12], 30)
    assert z == 0 and r <= ULP and bad > BAD
    # each column from the stored columns before it: the same columns when those are the exact ones
    cg, tg = s64.pchol_columns_given(A, s64.pchol64(A, np.diag(A), [], 7, 0.0)[3], cols[:7], cols[7:12], piv[7:12], 0.0)
    assert np.allclose(cg, cols[7:12], atol=1e-12) and np.allclose(tg, terms[7:12], rtol=1e-9)
    # ties: lower rank first; a pivot at or below tol_abs leaves a zero column; `allowed` ends the batch
    D = np.diag([1.0, 2.0, 2.0, 1e-9])
    assert s64.pchol64(D, np.diag(D), [], 4, 1e-6)[0] == [1, 2, 0, 3]
    pv, cl, _, _, _ = s64.pchol64(D, np.diag(D), [], 4, 1e-6, rank=[3, 2, 1, 0])
    assert pv == [2, 1, 0, 3] and np.all(cl[3] == 0) and np.isclose(cl[0][2], np.sqrt(2.0), rtol=1e-15)
    assert s64.pchol64(D, np.diag(D), [], 4, 1e-6, allowed={1, 2})[0] == [1, 2]
    assert s64.top_candidates([1.0, 2.0, 2.0, 0.5], 3) == [1, 2, 0] and s64.top_candidates([1.0, 2.0, 2.0, 0.5], 2, rank=[0, 3, 1, 2]) == [2, 1]


def test_dispatch_rules():
    assert s64.final_family(1024) == s64.final_family(3072) == "coldot_final_kernel/tail"
    assert s64.final_family(3073) == "coldot_final_kernel/unrolled"
    assert s64.direction_family("cg", 4099, 3, True) == "step_direction_kernel/cg"
    assert s64.direction_family("cg", 4100, 3, True) == "step_direction_vec_kernel/cg"
    assert s64.direction_family("pcg", 4100, 16, False) == "step_direction_kernel/pcg"
    assert s64.direction_family("pcg", 0, 4, True) == "step_direction_kernel/pcg"
    assert s64.gram_families(16, False) == ["pcg_gram_kernel<1,f32>"]
    assert s64.gram_families(144, True) == ["pcg_gram_kernel<8,f16>", "pcg_gram_kernel<1,f16>"]
    assert s64.gram_families(400, False) == ["pcg_gram_kernel<8,f32>"] * 3 + ["pcg_gram_kernel<1,f32>"]
    assert s64.rz_rows(1_100_000, False) == 4297 and s64.rz_rows(513, True) == 2
    assert [s64.lanczos_span(n) for n in (1, 65_536, 65_537, 262_144, 262_145, 1_048_576, 1_048_577, 2_097_152, 2_097_153)] == \
        [256, 256, 1024, 1024, 4096, 4096, 8192, 8192, None]
    for fams in (s64.coldot_families("cg_update_kernel/alpha"), s64.project_families(1008, True), s64.apply_families(5, 16, True, True),
                 s64.pchol_batch_families(3, 7, 7, 1), s64.lanczos_families(70_000), [s64.fused_family("cg_step_update_fused_kernel", 12)]):
        assert set(fams) <= set(s64.FAMILIES), fams


def test_solver_families_name_every_kernel_and_template_value():
    """Every __global__ kernel of plx_linalg.hip, plx_cg_kernels.h, plx_pcg.hip and plx_lanczos_kernels.h (but the two backward
    kernels DESIGN section 10 owns) and every template value their switch statements and PLX_*_CASE lists dispatch is a family of
    solver64.FAMILIES, and FAMILIES names no kernel the sources do not have: a new kernel or value fails here until a case
    reaches it."""
    kernels, pairs = s64.parse_sources()
    assert len(kernels) >= 26 and len(pairs) >= 52      # (26: the CG vector steps are five templated kernels, once)
    ours = kernels - set(s64.NOT_OURS)
    named = {s64.family_kernel(f) for f in s64.FAMILIES}
    assert named == ours, {"in the sources only": sorted(ours - named), "in FAMILIES only": sorted(named - ours)}
    have = {(s64.family_kernel(f), v) for f in s64.FAMILIES for v in s64.family_values(f)}
    assert pairs <= have, sorted(pairs - have)
    assert have <= pairs, sorted(have - pairs)
    assert len(s64.UNREACHABLE) <= 3 and set(s64.UNREACHABLE) <= set(s64.FAMILIES)
    # the templated Lanczos source: the fp32 ladder is the table's, and no type's ladder holds a span it has no rows for
    spans = s64.ladder_spans()
    assert spans["float"] == list(s64.LZ_SPANS) and spans["double"] == [256, 1024, 4096]
