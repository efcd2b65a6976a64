#!/usr/bin/env python3
"""d up to 32 and orders up to 8 (PLX_MAX_ORDER) against float64 (tests/lattice64.py): the one-shot filter and a many-MVM
build with the Morton vertex numbering forced.  Per entry |got - want| / terms64 and rel-L2.  The fixed cases also run in
the suite (tests/test_forward_fp64.py::test_extreme_shapes); this script takes extra (n, d, vd, order) cases as
arguments, e.g. 3000,32,7,8."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from tests.lattice64 import Lattice64, entry_ratio, rel_l2
from tests.test_forward_fp64 import EXTREME, gauss_taps

cases = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or EXTREME
rng = np.random.default_rng(1)
worst = (0.0, 0.0)
for (n, d, vd, order) in cases:
    ref = (rng.standard_normal((n, d)) * 0.8).astype(np.float32)
    src = rng.standard_normal((n, vd)).astype(np.float32)
    taps = gauss_taps(order)
    l64 = Lattice64(ref, taps)
    want = l64.apply(src) if n <= 3000 else l64.apply_staged(src)
    T = l64.terms64(src)
    got = plx.filter(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(taps)).cpu().numpy()
    nv.check(nv.lib().plx_tune(b"vertex_order", 2), "plx_tune")
    try:
        lat = plx.Lattice().build(torch.from_numpy(ref).cuda(), taps)
        got2 = lat.apply(torch.from_numpy(src).cuda()).cpu().numpy()
        assert lat.stage_kernels()["vertex_order"] == ["morton"] or lat.m < 2
        lat.close()
    finally:
        nv.check(nv.lib().plx_tune(b"vertex_order", 1), "plx_tune")
    for name, out in (("one-shot", got), ("morton", got2)):
        e, r = entry_ratio(out, want, T), rel_l2(out, want)
        worst = (max(worst[0], e), max(worst[1], r))
        print((n, d, vd, order), name, f"entry {e:.2e} of T, rel-L2 {r:.2e}", flush=True)
print(f"worst: entry {worst[0]:.2e} of T, rel-L2 {worst[1]:.2e}")
sys.exit(0 if worst[0] <= 1e-5 and worst[1] <= 1e-5 else 1)
