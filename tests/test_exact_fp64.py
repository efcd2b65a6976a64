"""The exact kernel MVM and its position gradient (plx_exact.hip) against float64 on the CPU, at every instantiation.

Every case calls the C ABI on fp32 data it made itself (tests/exact64.py: the case list, the data, the references) and
judges every output entry in units of its yardstick T, the terms the entry sums, each weighted by 1 + the magnitude of its
exponential's argument.  One pytest case is one group of exact64.CASES: a (kind, profile, DP) with both ends of the d
range, t at both ends of every TC and with one to three column blocks, n1 around the 256-row workgroup, n2 around the
128-row LDS tile, the ragged split shape, and the data kinds in rotation (a cloud, the cloud shifted by 30, coincident
points, a row too far for any term to reach FLT_MIN); the named split shapes are two more groups.
Every device array has exactly the stated size, starts at an odd float offset in its allocation and is followed by
sentinels; the workspace is exactly plx_exact_work_bytes.  Inputs come back bit-unchanged, a second call (on the used
workspace) is bit-equal to the first, the slabs of a split call are all written, an empty slice's as zeros.
test_every_family_was_reached (last) fails if one of the 224 instantiations or a required slab path did not run.

The bars are 4x the worst ratio measured on the MI355X per quantity (DESIGN.md section 9 has the table per kind and
profile), far under the ceiling of 2e-5 of T.  PLX_EXACT64_REPORT=<file> writes the worst ratio per family of a run as JSON."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import exact64 as x64
from tests.gpubuf import Buf, _bits_equal, check_buffers

pytestmark = pytest.mark.gpu

CEILING = 2e-5           # no bar may exceed this: about twice the bound of a sequential fp32 sum over a 128-row tile plus
                         # the DP + 8 roundings of a term (170 * 2^-24)
# quantity -> bar = 4 x the worst measured over all families
BAR = {
    "mvm": 2.7e-6,           # forward entry, |got - want| / T: worst 6.63e-7 (rbf, DP = 20, TC = 16)
    "grad": 1.6e-6,          # gradient entry: worst 4.01e-7 (matern12, DP = 32, TC = 4)
}
WORST = {}               # family (kind, profile, DP, TC, path) -> worst ratio
OFFSETS = dict(x1=1, x2=3, v=5, g=7, out=3, work=1)      # floats into the allocation: nothing may assume 16-byte alignment


@pytest.fixture(scope="module")
def lib():
    import simplex_gp_amd  # noqa: F401
    from simplex_gp_amd import _native as nv
    assert torch.cuda.is_available()
    return nv.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, c, X1, X2, G, V, out, work, work_bytes):
    prof = x64.PROFILES.index(c.profile)
    if c.kind == "mvm":
        rc = lib.plx_exact_mvm(X1.ptr, c.n1, X2.ptr, c.n2, c.d, prof, V.ptr, c.t, out.ptr, work.ptr, work_bytes, stream())
    else:
        rc = lib.plx_exact_grad(X1.ptr, c.n1, X2.ptr, c.n2, c.d, prof, G.ptr, V.ptr, c.t, out.ptr, work.ptr, work_bytes, stream())
    assert rc == 0, (c, rc, lib.plx_last_error())
    torch.cuda.synchronize()


def run_case(lib, c):
    data = x64.make_data(c)
    splits = lib.plx_exact_splits(c.n1, c.n2, c.d, c.t)
    fam = x64.family(c.kind, c.profile, c.d, c.t, splits)
    work_bytes = lib.plx_exact_work_bytes(c.n1, c.n2, c.d, c.t)
    assert work_bytes > 0 and work_bytes % 4 == 0
    width = c.t if c.kind == "mvm" else c.d
    X1, X2, V = (Buf(data[k], offset=OFFSETS[k]) for k in ("x1", "x2", "v"))
    G = Buf(data["g"], offset=OFFSETS["g"]) if c.kind == "grad" else None
    inputs = [b for b in (X1, X2, V, G) if b is not None]
    out, again = Buf(count=c.n1 * width, offset=OFFSETS["out"]), Buf(count=c.n1 * width, offset=OFFSETS["out"])
    work = Buf(count=work_bytes // 4, offset=OFFSETS["work"])              # sentinels throughout
    call(lib, c, X1, X2, G, V, out, work, work_bytes)
    check_buffers(inputs, [out, work])
    if splits > 1:
        used = splits * c.n1 * width
        assert 4 * used <= work_bytes, (c, splits)
        slabs = work.cpu()[:used].reshape(splits, c.n1 * width)
        chunk = -(-c.n2 // splits)
        empty = [s for s in range(splits) if s * chunk >= c.n2]
        assert not bool((slabs == work.sent).any()), ("a slab entry was never written", c)
        assert all(bool((slabs[s] == 0).all()) for s in empty), ("the slab of an empty slice is not zero", c)
    call(lib, c, X1, X2, G, V, again, work, work_bytes)
    check_buffers(inputs, [again, work])
    got = out.cpu()
    assert _bits_equal(got, again.cpu()), ("two identical calls differ", c)
    got = got.numpy().reshape(c.n1, width)
    if c.kind == "mvm":
        want, T = x64.mvm64(data["x1"], data["x2"], data["v"], c.profile)
        floor = x64.mvm_floor(c.n2, data["v"])
    else:
        want, T = x64.grad64(data["x1"], data["x2"], data["g"], data["v"], c.profile)
        floor = x64.grad_floor(data["x1"], data["x2"], data["g"], data["v"])
    ratio = x64.entry_ratio(got, want, T, floor)
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    print(f"{ratio:9.2e}  {'|'.join(map(str, fam))}  d={c.d} t={c.t} n1={c.n1} n2={c.n2} {c.data} splits={splits}")
    return ratio


@pytest.mark.parametrize("group", x64.GROUPS)
def test_exact_against_fp64(lib, group):
    """every case of the group; the figures are printed before anything is asserted on them"""
    cases = [c for c in x64.CASES if c.group == group]
    ratios = [run_case(lib, c) for c in cases]
    for c, ratio in zip(cases, ratios):
        assert ratio <= BAR[c.kind], (c, ratio, BAR[c.kind])


def test_every_family_was_reached():
    """Acceptance: all 224 instantiations ran, and the slab path at every TC of the forward and every DP of the gradient,
    for every profile.
    Run the module whole: pytest -m gpu tests/test_exact_fp64.py"""
    path = os.environ.get("PLX_EXACT64_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"|".join(map(str, fam)): v for fam, v in sorted(WORST.items())}, f, indent=1)
    if len(WORST) == 0:
        pytest.fail("no case of this module ran before the acceptance test")
    assert all(0 < bar <= CEILING for bar in BAR.values())
    assert x64.missing_coverage(WORST) == []
    for fam, v in sorted(WORST.items()):
        assert v <= BAR[fam[0]], (fam, v)
    assert np.isfinite(list(WORST.values())).all()
