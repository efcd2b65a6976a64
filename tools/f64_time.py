"""Time the float64 lattice product (plx_apply_f64) next to the fp32 product of the same build.

Method: device events around `calls` back-to-back products, the minimum over `rounds` rounds, fp32 and fp64 alternating
round by round in one process on one lattice, after a warm-up of both (tables, workspaces, code objects).  The fp64 stages
are timed one by one the same way.  Next to every time: the bytes the product has to move, counted from the shapes --
what an ideal implementation reads and writes once per stage (value rows, index and weight tables, the caller's rows), not
what the caches actually served.

    python tools/f64_time.py [--out profiles/f64_measured.md] [--rounds 7] [--calls 20]

Shapes: N = 1e6, d = 8, order 1, x ~ N(0, I) from seed 1234 (the headline build) at vd in {1, 12, 101}; the config-5
stand-in (MaternLattice nu = 1.5, order 3, N = 10,623, d = 18) at vd = 1.  Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402


def product_bytes(n, m, d, order, vd, elem):
    """Bytes one product moves at least, per stage: (splat, blur, slice).  elem = 4 (fp32) or 8 (fp64); the value-row
    stride is vd rounded up to 16 bytes (1 element for vd = 1)."""
    per16 = 16 // elem
    stride = 1 if vd == 1 else (vd + per16 - 1) // per16 * per16
    nnz = n * (d + 1)
    splat = nnz * 8 + n * vd * elem + m * stride * elem                    # corner row + weight, source rows, vertex rows out
    blur = (d + 1) * (2 * m * stride * elem + 2 * order * m * 4)           # per axis: rows in and out, the neighbour ids
    slice_ = nnz * 8 + m * stride * elem + n * vd * elem + n * 4           # entry ids + weights, vertex rows, rows out, permutation
    return splat, blur, slice_


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def measure(lat, v32, rounds, calls):
    vd = v32.shape[1]
    v64 = v32.double()
    o32, o64 = torch.empty_like(v32), torch.empty_like(v64)
    val = lat.new_values(vd, torch.float64)
    tmp = torch.empty_like(val)
    runs = {
        "fp32": lambda: lat.apply(v32, o32),
        "fp64": lambda: lat.apply(v64, o64),
        "fp64 splat": lambda: lat.splat(v64, val),
        "fp64 blur": lambda: lat.blur(val, tmp, vd=vd),
        "fp64 slice": lambda: lat.slice(val, o64, vd=vd),
    }
    for fn in runs.values():                                  # warm-up: tables, workspaces, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():                            # alternating: every round times every variant once
            best[k] = min(best[k], timed(fn, calls))
    want = lat.apply(v64)                                     # (o64 has been overwritten by the staged slice)
    rel = float((lat.apply(v32).double() - want).norm() / want.norm())
    return best, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda", 0)
    shapes = []
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1_000_000, 8, generator=g).to(dev)
    shapes.append(("N = 1e6, d = 8, order 1", x, np.array([0.34608543, 1.0, 0.34608543], np.float32), (1, 12, 101)))
    g = torch.Generator().manual_seed(1234)
    x5 = torch.randn(10623, 18, generator=g).to(dev)
    taps5 = plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18).dkernel_fn.get_coeffs().numpy()
    shapes.append(("N = 10,623, d = 18, order 3 (config-5 stand-in)", x5, taps5, (1,)))
    lines = ["| shape | vd | m | fp32 ms | fp32 MB | fp64 ms | fp64 MB | fp64 / fp32 time | fp64 / fp32 bytes | "
             "fp64 splat / blur / slice ms | fp64 splat / blur / slice MB | rel-L2 fp32 vs fp64 |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for name, x, taps, vds in shapes:
        lat = plx.Lattice(dev).build(x, taps)
        n, d = x.shape
        rows = np.diff(lat.export(plx._native.ARRAY_ROW_PTR).astype(np.int64))
        print(f"{name}: m = {lat.m}, corners per vertex row: mean {rows.mean():.1f}, median {int(np.median(rows))}, "
              f"max {int(rows.max())}", flush=True)
        notes.append(f"- {name}: m = {lat.m}; corners per vertex row: mean {rows.mean():.1f}, median "
                     f"{int(np.median(rows))}, max {int(rows.max())}")
        for vd in vds:
            v = torch.randn(n, vd, generator=torch.Generator().manual_seed(vd)).to(dev)
            best, rel = measure(lat, v, args.rounds, args.calls)
            b32 = product_bytes(n, lat.m, d, lat.order, vd, 4)
            b64 = product_bytes(n, lat.m, d, lat.order, vd, 8)
            lines.append(
                f"| {name} | {vd} | {lat.m} | {best['fp32']:.3f} | {sum(b32) / 1e6:.1f} | {best['fp64']:.3f} | "
                f"{sum(b64) / 1e6:.1f} | {best['fp64'] / best['fp32']:.2f} | {sum(b64) / sum(b32):.2f} | "
                f"{best['fp64 splat']:.3f} / {best['fp64 blur']:.3f} / {best['fp64 slice']:.3f} | "
                f"{b64[0] / 1e6:.1f} / {b64[1] / 1e6:.1f} / {b64[2] / 1e6:.1f} | {rel:.1e} |")
            print(lines[-1], flush=True)
        lat.close()
    text = (f"device: {torch.cuda.get_device_name(0)}; minimum of {args.rounds} rounds of {args.calls} calls, device events, "
            "fp32 and fp64 alternating\n\n" + "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
