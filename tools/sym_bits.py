"""Dump the bits of the transposed and the symmetrised lattice products for the library PLX_LIBRARY names (default: the
tree's libplx.so), to compare two builds of the library byte for byte:

    PLX_LIBRARY=/path/to/libplx.so python tools/sym_bits.py > dump.txt        (one process per library, then cmp)

The fp32 calls run over the CASES of tests/test_sym_gpu.py, the float64 ones over the CASES of tests/test_sym_f64_gpu.py, on
the inputs those modules build (the same clouds, taps, seeds, sizes, row orders and buffer alignment).  Six calls per case:
blur_t_f32, blur_sym_f32, apply_t_f32, apply_sym_f32, apply_affine_sym_f32 and apply_affine_sym_f32(want_dot=True) where
the width allows the fused dot (2..256 columns); in float64 blur_t, blur_sym, apply_t, apply_sym, apply_affine(symmetric=
True) and the same with want_dot=True where affine_dot_f64_ok (apply_affine(symmetric=True) itself is float64 only).  One
line per output, the dots included: the case id, the call, the kernels it reported, the byte count, the SHA-256 of the bytes
and the count of non-finite values.  The last line names the kernels seen.  Needs a GPU.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from tests import test_sym_f64_gpu as t64  # noqa: E402
from tests import test_sym_gpu as t32  # noqa: E402
from tests.lattice64 import cloud  # noqa: E402
from tests.sym64 import taps_of  # noqa: E402

SCALE_SHIFT = (1.5, -0.25)


def emit(tag, case_id, call, lat, kernels, seen, outs):
    torch.cuda.synchronize()
    k = getattr(lat, kernels)()
    names = "+".join(k["splat"] + k["blur"] + k["slice"])
    seen.update(k["splat"] + k["blur"] + k["slice"])
    for what, t in outs:
        raw = t.contiguous().cpu().numpy().tobytes()
        bad = int((~torch.isfinite(t)).sum())
        print(f"{tag} {case_id} {call}{what} {names} {len(raw)} {hashlib.sha256(raw).hexdigest()} nonfinite={bad}", flush=True)


def run(tag, mod, f64, seen):
    dtype, kernels = (np.float64, "sym_f64_kernels") if f64 else (np.float32, "sym_kernels_f32")
    lats = {}
    for case, case_id in zip(mod.CASES, mod.IDS):
        kind, n, d, order, lop, vd, aligned = case[:7]
        lrows = False if f64 else case[7]
        key = (kind, n, d, order, lop)
        if key not in lats:
            taps = taps_of(order, lop)
            x = cloud(kind, n, d, seed=3 + d + order, coeffs=taps)        # the points of test_sym_f64_gpu.operator
            lats[key] = plx.Lattice().build(mod.cuda(x, np.float32), taps)
        lat = lats[key]
        v = np.random.default_rng(vd + 11 * d).standard_normal((n, vd)).astype(dtype)
        if kind == "isolated":
            v[::2] = 0.0
        ss = torch.tensor(SCALE_SHIFT, dtype=torch.float64 if f64 else torch.float32, device="cuda")
        lat.set_lattice_row_order(lrows)
        try:
            src = mod.placed(n, vd, aligned, lat.to_lattice_order(mod.cuda(v, dtype)) if lrows else mod.cuda(v, dtype))
            out = lambda: mod.placed(n, vd, aligned)        # noqa: E731
            V = lat.splat(src)
            if f64:
                stages = (("blur_t", lambda: lat.blur_t(V.clone(), vd=vd)), ("blur_sym", lambda: lat.blur_sym(V.clone(), vd=vd)),
                          ("apply_t", lambda: lat.apply_t(src, out=out())), ("apply_sym", lambda: lat.apply_sym(src, out=out())),
                          ("apply_affine_sym", lambda: lat.apply_affine(src, ss, out=out(), symmetric=True)))
                dot_ok = lat.affine_dot_f64_ok(vd)
                with_dot = lambda: lat.apply_affine(src, ss, out=out(), want_dot=True, symmetric=True)        # noqa: E731
            else:
                stages = (("blur_t_f32", lambda: lat.blur_t_f32(V.clone(), vd=vd)),
                          ("blur_sym_f32", lambda: lat.blur_sym_f32(V.clone(), vd=vd)),
                          ("apply_t_f32", lambda: lat.apply_t_f32(src, out=out())),
                          ("apply_sym_f32", lambda: lat.apply_sym_f32(src, out=out())),
                          ("apply_affine_sym_f32", lambda: lat.apply_affine_sym_f32(src, ss, out=out())))
                dot_ok = 2 <= vd <= 256
                with_dot = lambda: lat.apply_affine_sym_f32(src, ss, out=out(), want_dot=True)        # noqa: E731
            for call, fn in stages:
                emit(tag, case_id, call, lat, kernels, seen, (("", fn()),))
            if dot_ok:
                res, dot = with_dot()
                emit(tag, case_id, "affine_sym_dot", lat, kernels, seen, ((".out", res), (".dot", dot)))
        finally:
            lat.set_lattice_row_order(False)
    for lat in lats.values():
        lat.close()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("sym_bits.py needs a GPU")
    seen = set()
    run("f32", t32, False, seen)
    run("f64", t64, True, seen)
    print("kernels " + " ".join(sorted(seen)))


if __name__ == "__main__":
    main()
