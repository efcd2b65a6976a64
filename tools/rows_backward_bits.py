"""Dump the bits of the one-sided position gradient of the rectangular product for the library PLX_LIBRARY names (default:
the tree's libplx.so), to compare two builds of the library byte for byte:

    PLX_LIBRARY=/path/to/libplx.so python tools/rows_backward_bits.py > dump.txt        (one process per library, then diff)

Lattice.apply_backward_rows_f32 runs over the 13 CASES of tests/rows_backward32.py and Lattice.apply_backward_rows over the
CASES of tests/rows_backward64.py (the list of tests/test_rows_backward_f64_gpu.py), on the inputs those modules build (N = 701
points, the same seeds, the same buffer alignment), both one-sided calls of each case: (a, b) and (b, a).  One line per
output, grad_x and filtered: the case id, the kernels the call reported, the byte count, the SHA-256 of the bytes and the
count of non-finite values.  The last line names the kernels seen; all eight must be there.  Needs a GPU.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from tests import rows_backward32, rows_backward64  # noqa: E402
from tests.lattice64 import cloud  # noqa: E402
from tests.test_backward_f64_gpu import dkernel, positions64  # noqa: E402
from tests.test_rows_fp64 import ranges  # noqa: E402

N = 701


def placed(a, dtype, aligned):
    """`a` as a contiguous CUDA tensor whose data pointer is 16-byte aligned, or that plus one element."""
    a = np.ascontiguousarray(a, dtype)
    off = 0 if aligned else 1
    buf = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def inputs32(idx, case):
    d, L, order, profile, kind, aligned, rname = case
    dtaps = dkernel(profile, order).get_deriv_coeffs().numpy()
    x = cloud(kind, N, d, seed=idx + 1, coeffs=dtaps)
    rng = np.random.default_rng(3000 + idx)
    return x, x, dtaps, rng


def inputs64(idx, case):
    d, L, order, profile, kind, aligned, rname = case
    dtaps = dkernel(profile, order).get_deriv_coeffs().numpy()
    x = positions64(kind, N, d, seed=idx + 1, coeffs=dtaps)
    rng = np.random.default_rng(2000 + idx)
    return x, x.astype(np.float32), dtaps, rng


def run(tag, cases, ids, inputs, dtype, call, kernels, seen):
    for idx, case in enumerate(cases):
        d, L, order, profile, kind, aligned, rname = case
        x, x_build, dtaps, rng = inputs(idx, case)
        (ab, ac), (bb, bc) = ranges(rname, N)
        a, b = rng.standard_normal((ac, L)), rng.standard_normal((bc, L))
        if kind == "isolated":
            a[::2] = 0.0
            b[::2] = 0.0
        lat = plx.Lattice().build(placed(x_build, np.float32, True), dtaps)
        ta, tb, tx = placed(a, dtype, aligned), placed(b, dtype, aligned), placed(x, dtype, aligned)
        for side, args in (("ab", (ta, ab, tb, bb)), ("ba", (tb, bb, ta, ab))):
            grad_x, filtered = getattr(lat, call)(*args, tx)
            torch.cuda.synchronize()
            k = getattr(lat, kernels)()
            names = "+".join(k["splat"] + k["slice"])
            seen.update(k["splat"] + k["slice"])
            for what, t in (("grad_x", grad_x), ("filtered", filtered)):
                raw = t.cpu().numpy().tobytes()
                bad = int((~torch.isfinite(t)).sum())
                print(f"{tag} {ids[idx]} {side} {what} {names} {len(raw)} {hashlib.sha256(raw).hexdigest()} nonfinite={bad}", flush=True)
        lat.close()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("rows_backward_bits.py needs a GPU")
    seen = set()
    run("f32", rows_backward32.CASES, rows_backward32.IDS, inputs32, np.float32, "apply_backward_rows_f32", "rows_kernels", seen)
    run("f64", rows_backward64.CASES, rows_backward64.IDS, inputs64, np.float64, "apply_backward_rows", "rows_f64_kernels", seen)
    print("kernels " + " ".join(sorted(seen)))


if __name__ == "__main__":
    main()
