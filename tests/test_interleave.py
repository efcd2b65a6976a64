"""tests/interleave.py without a GPU: the generator covers what it promises, the op table names every launching method of
Lattice, the scenario clouds meet the CPU-checkable conditions of their regimes, the backward shapes are served, and the
step checker rejects the wrong results it exists to catch."""
import numpy as np
import pytest

from oracle import oracle
from tests import interleave as il

SCENARIOS = sorted(il.SCENARIOS)


# ---- the generator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scn", SCENARIOS)
def test_generator_covers_firsts_and_pairs(scn):
    seqs = il.sequences(scn)
    assert seqs == il.sequences(scn), "deterministic"
    firsts = {k: set() for k in il.KINDS}
    pairs = set()
    for seq in seqs:
        assert 0 < len(il.steps_of(seq)) <= il.STEP_CAP
        for chain in seq:
            assert len(chain) == len(il.BUILDS) and chain[-1] == chain[0], "the last segment repeats the first"
            for build, seg in zip(il.BUILDS, chain):
                assert seg and all(name in il.OPS for name in seg)
                firsts[il.BUILD_KIND[build]].add(seg[0])
                for a, b in zip(seg, seg[1:]):
                    pairs.add((il.OPS[a].group, il.OPS[b].group))
                    if a == "row_order":
                        assert il.OPS[b].group in il.ROW_ORDER_GROUPS
                assert seg[-1] != "row_order"
    for kind in il.KINDS:
        assert firsts[kind] == set(il.OPS), (kind, sorted(set(il.OPS) - firsts[kind]))
    assert pairs == {(a, b) for a in il.GROUPS for b in il.GROUPS}


def test_scenarios_differ_in_their_sequences():
    assert len({repr(il.sequences(s)) for s in SCENARIOS}) == len(SCENARIOS)


# ---- completeness ------------------------------------------------------------------------------------------------------
def test_op_table_names_every_launching_method():
    """Every public method of Lattice that reaches a plx_* launch is run by some op (or is a build of the chain, one of the
    named exclusions, or composed of methods that are)."""
    import simplex_gp_amd as plx
    launching = il.launching_methods()
    assert {"apply", "apply_rows", "diag", "locate", "slice_at", "export", "shard_perm", "apply_at", "to_lattice_order",
            "build_local", "filter_once"} <= launching, "the parse of lattice.py lost methods it must find"
    assert all(hasattr(plx.Lattice, m) for m in launching)
    covered = {m for o in il.OPS.values() for m in o.methods}
    assert all(hasattr(plx.Lattice, m) for m in covered)
    for name, parts in il.COMPOSED_METHODS.items():
        assert all(p in covered or p in il.COMPOSED_METHODS for p in parts), name
    missing = launching - covered - il.BUILD_METHODS - il.EXCLUDED_METHODS - set(il.COMPOSED_METHODS)
    assert not missing, ("Lattice methods that launch work and that no op runs", sorted(missing))
    assert {o.group for o in il.OPS.values()} == set(il.GROUPS)


def test_no_exception_names_an_op():
    """The table of intended history dependence is empty: plx.h promises bit-equal repeat calls for every entry point here."""
    for (earlier, name), why in il.INTENDED_DEPENDENCE.items():
        assert earlier in il.OPS and name in il.OPS and ":" in why


# ---- regimes -----------------------------------------------------------------------------------------------------------
def _structure(ref):
    oracle.set_exact_mode(False)
    try:
        lat = oracle.Lattice(ref.x, ref.taps)
    finally:
        oracle.set_exact_mode(True)
    try:
        return int(lat.m), float((lat.neighbors() >= 0).mean())
    finally:
        lat.close()


def test_regime_conditions_hold_for_the_clouds():
    got = {}
    for scn in SCENARIOS:
        ref = il.refs(scn)["cold"]
        m, occupancy = _structure(ref)
        got[scn] = (m, ref.n * (ref.d + 1), occupancy)
    print(got)
    m, nnz, _ = got["coarse"]
    assert 2 * m <= nnz                                           # block tables: the first gate
    m, nnz, _ = got["mid"]
    assert 2 * m > nnz and 10 * (nnz - m) > nnz and m <= 16384    # neither the block path nor the first-touch path
    m, nnz, _ = got["fine"]
    assert 10 * (nnz - m) <= nnz and nnz > m and m <= 16384       # first touch, with extras
    m, nnz, occ = got["fine-large"]
    assert m > 16384 and occ < 0.25 and 10 * (nnz - m) <= nnz and nnz > m
    m, nnz, occ = got["mid-large"]
    assert m > 16384 and occ >= 0.25 and 2 * m > nnz and 10 * (nnz - m) > nnz
    for scn in SCENARIOS:                                         # the other cloud is another n and another d
        s = il.SCENARIOS[scn]
        assert abs(s["other"][0] - s["n"]) == 1 and s["other"][1] != s["d"]
    assert sorted(il.SCENARIOS[s]["other"][0] - il.SCENARIOS[s]["n"] for s in il.SCENARIOS) == [-1, -1, 1, 1, 1]


def test_backward_shapes_are_served():
    import simplex_gp_amd as plx
    ds = {s["d"] for s in il.SCENARIOS.values()} | {s["other"][1] for s in il.SCENARIOS.values()}
    assert ds <= set(il.BACKWARD_NRHS)
    for d in ds:
        assert plx.Lattice.backward_fusable(il.BACKWARD_NRHS[d], d), d
        assert plx.Lattice.backward_f64_ok(il.F64_NRHS, d)
        assert plx.Lattice.backward_rows_ok(il.ROWS_NRHS, d) and plx.Lattice.backward_rows_f64_ok(il.ROWS_NRHS, d)


# ---- the checker -------------------------------------------------------------------------------------------------------
OP, VD, TAG = "apply_vd11", 11, "a11"


@pytest.fixture(scope="module")
def synthetic():
    """A "device result" of apply_vd11 on the fine scenario made from the float64 reference, and that reference."""
    rf = il.refs("fine")
    ref = rf["cold"]
    v = ref.rhs(TAG, ref.n, VD)
    want, T = il.fwd_reference(ref, v)
    return rf, ref, v, want, T, want.astype(np.float32)


def rejected(ref, res, twin=None, match="float64 bar"):
    with pytest.raises(AssertionError, match=match):
        il.check_step(OP, ref, res, twin)


def test_checker_accepts_the_rounded_reference(synthetic):
    rf, ref, v, want, T, good = synthetic
    items = il.check_step(OP, ref, {"out": good}, {"out": good.copy()})
    assert items and all(r <= 0.1 for _, r in items)


def test_checker_rejects_one_entry_moved_by_four_bars(synthetic):
    from tests.test_forward_fp64 import ENTRY
    rf, ref, v, want, T, good = synthetic
    bad = good.copy()
    i, j = ref.n // 2, 7
    bad[i, j] = np.float32(want[i, j] + 4 * ENTRY * T[i, j])
    assert bad[i, j] != good[i, j]
    rejected(ref, {"out": bad})


def test_checker_rejects_two_rows_swapped(synthetic):
    rf, ref, v, want, T, good = synthetic
    bad = good.copy()
    bad[[3, 4]] = bad[[4, 3]]
    rejected(ref, {"out": bad})


def test_checker_rejects_the_previous_builds_operator(synthetic):
    """The stale-table case: the operator of the warm rebuild (1.05 x) applied to the same input."""
    rf, ref, v, want, T, good = synthetic
    stale = rf["warm"].l64.apply_staged(v).astype(np.float32)
    rejected(ref, {"out": stale})


def test_checker_rejects_a_column_taken_from_its_neighbour(synthetic):
    """Column 10 of 11 sits beside the padding column of the 12-wide vertex row."""
    rf, ref, v, want, T, good = synthetic
    bad = good.copy()
    bad[:, VD - 1] = bad[:, VD - 2]
    rejected(ref, {"out": bad})


def test_checker_rejects_one_bit_off_the_twin(synthetic):
    rf, ref, v, want, T, good = synthetic
    twin = good.copy()
    twin[11, 2] = np.nextafter(twin[11, 2], np.float32(np.inf))
    il.check_step(OP, ref, {"out": twin})                   # within the bar on its own
    rejected(ref, {"out": good}, {"out": twin}, match="differs from the fresh twin")
    with pytest.raises(AssertionError, match="kernel families"):
        il.check_step(OP, ref, {"out": good}, {"out": good.copy()}, {"splat": ["a"]}, {"splat": ["b"]})
    with pytest.raises(AssertionError, match="revisit"):
        il.check_step(OP, ref, {"out": good}, first={"out": twin})
