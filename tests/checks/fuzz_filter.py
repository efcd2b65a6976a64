#!/usr/bin/env python3
"""Wide randomised comparison of the HIP filter against float64 (tests/lattice64.py: the oracle's duplicate-free structure,
every sum in float64): shapes up to n = 6000, d = 12, column counts that hit every splat / blur / slice kernel, all tap
orders, degenerate clouds, with the compacted neighbour table forced on a third of the cases; odd cases go through build()
+ apply() with the Morton vertex numbering and both two-axes-per-launch blurs forced on, even ones through the one-shot
plx_filter (first-touch numbering).  Bars: per entry |got - want| <= 1e-5 terms64 (the size of the terms the entry sums:
no allowance for cancellation is needed) and rel-L2 <= 1e-5.  30 fixed-seed cases of the same generator run in the suite
(tests/test_forward_fp64.py::test_fuzz_fixed_seed)."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from tests.lattice64 import Lattice64, entry_ratio, rel_l2
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
VD = [1, 1, 2, 3, 4, 5, 6, 7, 9, 12, 13, 16, 17, 31, 33, 60, 64, 65, 100, 124, 126, 130, 198, 260]
worst = (0.0, 0.0, None)
for c in range(cases):
    n = int(rng.choice([1, 2, 3, 17, 64, 65, 255, 257, 1000, 2049, 6000]))
    d = int(rng.integers(1, 13))
    vd = int(rng.choice(VD))
    order = int(rng.integers(0, 4))
    scale = float(rng.choice([0.02, 0.3, 1.0, 4.0, 30.0]))
    kind = str(rng.choice(["normal", "grid", "dup", "line", "same"]))
    if kind == "normal":
        ref = rng.standard_normal((n, d))
    elif kind == "grid":
        ref = rng.integers(-3, 4, (n, d)).astype(np.float64) * 0.5
    elif kind == "dup":
        k = max(1, n // 20)
        ref = rng.standard_normal((k, d))[rng.integers(0, k, n)]
    elif kind == "line":
        ref = np.outer(rng.standard_normal(n), rng.standard_normal(d))
    else:
        ref = np.tile(rng.standard_normal((1, d)), (n, 1))
    ref = (ref * scale).astype(np.float32)
    src = rng.standard_normal((n, vd)).astype(np.float32)
    taps = np.array([0.1, 0.3, 0.6, 1.0, 0.6, 0.3, 0.1][3 - order: 4 + order], np.float32)
    nv.check(nv.lib().plx_tune(b"compact_nbr", 2 if c % 3 == 0 else 1), "plx_tune")
    if c % 2:
        nv.check(nv.lib().plx_tune(b"vertex_order", 2), "plx_tune")
        nv.check(nv.lib().plx_tune(b"blur_fuse", 2), "plx_tune")
        lat = plx.Lattice().build(torch.from_numpy(ref).cuda(), taps)
        out = lat.apply(torch.from_numpy(src).cuda()).cpu().numpy()
        lat.close()
        nv.check(nv.lib().plx_tune(b"vertex_order", 1), "plx_tune")
        nv.check(nv.lib().plx_tune(b"blur_fuse", 1), "plx_tune")
    else:
        out = plx.filter(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), taps).cpu().numpy()
    l64 = Lattice64(ref, taps)
    want = l64.apply(src) if n <= 3000 else l64.apply_staged(src)
    e, r = entry_ratio(out, want, l64.terms64(src)), rel_l2(out, want)
    if e > worst[0]:
        worst = (e, worst[1], (n, d, vd, order, scale, kind, c))
    worst = (worst[0], max(worst[1], r), worst[2])
    if e > 1e-5 or r > 1e-5:
        print(f"case {c}: entry {e:.2e} of T, rel-L2 {r:.2e}", (n, d, vd, order, scale, kind), "FAIL", flush=True)
        sys.exit(1)
nv.check(nv.lib().plx_tune(b"compact_nbr", 1), "plx_tune")
print(f"{cases} cases, worst entry {worst[0]:.2e} of T at (n, d, vd, order, scale, kind, case) = {worst[2]}, "
      f"worst rel-L2 {worst[1]:.2e}")
