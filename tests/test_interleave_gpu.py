"""Every Lattice entry point interleaved on one object per scenario, at the shipped switches (tests/interleave.py).

One case is one generated sequence: a few chains of five builds (cold, warm, cold on another cloud, filter_once, cold again)
on the scenario's ONE Lattice, a few ops after each.  Every step is held to (a) the float64 reference and the bar of the op's
own test module, (b) the bits and the kernel names of a fresh twin that made only the builds since the last cold one,
(c) the guard elements of its buffers, (d) in the last segment, the bits of the first.  The module forces no kernel family:
after a scenario's last sequence test_regime asserts that the path the scenario is named for was really taken, and that no
generated step was skipped.  The worst ratio to its bar per op and scenario is printed at the end (pytest -s) and copied to
profiles/interleave_measured.md.
"""
import pytest

from simplex_gp_amd import _native as nv
from tests import interleave as il
from tests import test_forward_fp64 as fwd
from tests.test_hip_parity import ROUND5_BUILD_DEFAULTS

pytestmark = pytest.mark.gpu

SEQUENCES = {scn: il.sequences(scn) for scn in il.SCENARIOS}
CASES = [(scn, i) for scn in il.SCENARIOS for i in range(len(SEQUENCES[scn]))]
_RUNNERS = {}


@pytest.fixture(scope="module", autouse=True)
def shipped_switches():
    """The process at the shipped switches, and left there."""
    for k, v in dict(fwd.DEFAULTS, **ROUND5_BUILD_DEFAULTS).items():
        nv.check(nv.lib().plx_tune(k.encode(), int(v)), "plx_tune")
    yield
    for r in _RUNNERS.values():
        r.close()
    report()


def runner(scn):
    if scn not in _RUNNERS:
        _RUNNERS[scn] = il.Runner(scn)
    return _RUNNERS[scn]


def report():
    if not _RUNNERS:
        return
    scns = [s for s in il.SCENARIOS if s in _RUNNERS]
    print("\ninterleaved entry points: worst ratio to the op's own float64 bar, per op and scenario")
    print(f"{'op':<24} {'group':<5} " + " ".join(f"{s:>10}" for s in scns))
    for name in ["filter_once"] + list(il.OPS):
        cells = " ".join(f"{_RUNNERS[s].worst[name]:10.3f}" if name in _RUNNERS[s].worst else f"{'-':>10}" for s in scns)
        print(f"{name:<24} {il.OPS[name].group if name in il.OPS else 'build':<5} {cells}")
    print("steps run: " + ", ".join(f"{s} {_RUNNERS[s].steps_run}" for s in scns))


@pytest.mark.parametrize("scn,i", CASES, ids=[f"{s}-{i:02d}" for s, i in CASES])
def test_sequence(scn, i):
    runner(scn).run(SEQUENCES[scn][i], label=f"{scn}-{i:02d}")


def _names(kern, stage):
    return "+".join(kern[stage])


@pytest.mark.parametrize("scn", list(il.SCENARIOS))
def test_regime(scn):
    """After the scenario's last sequence: every generated step ran, and the shipped gates picked the path of the table."""
    r = runner(scn)
    assert r.steps_run == sum(len(il.steps_of(seq)) for seq in SEQUENCES[scn]), "a generated step was skipped"
    assert not il.INTENDED_DEPENDENCE
    single = r.kernels_seen[("again", "apply_vd1")] if ("again", "apply_vd1") in r.kernels_seen else r.kernels_seen[("cold", "apply_vd1")]
    back = r.kernels_seen.get(("again", "backward_f32"), r.kernels_seen.get(("cold", "backward_f32")))
    splat, blur = _names(single, "splat"), _names(single, "blur_axis")
    print(scn, "vd = 1:", single, " fused backward:", back, " block rows:", r.block_rows)
    regime = il.SCENARIOS[scn]["regime"]
    if regime == "block":
        assert r.block_rows > 0 and splat == fwd.BLOCK and blur == fwd.SMALL
    elif regime == "csr":
        assert r.block_rows == 0 and splat == fwd.SCAN and blur == fwd.SMALL
    elif regime == "first":
        assert splat in (fwd.FIRST_X, fwd.FIRST_SEQ_X) and blur == fwd.SMALL
    elif regime == "compact":
        assert splat in (fwd.FIRST_X, fwd.FIRST_SEQ_X) and blur == fwd.COMPACT
        assert _names(back, "blur_axis") == fwd.ACTIVE
    else:
        assert regime == "pair" and splat == fwd.SCAN and blur == fwd.PAIR_V1_ODD
        assert _names(back, "blur_axis") != fwd.ACTIVE
