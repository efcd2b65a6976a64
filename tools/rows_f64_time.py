"""Time the float64 rectangular product K(x*, X) V: the native row-range route (plx_apply_rows_f64) against the padded square
filter that RectangularLazyLattice runs with native_rows_f64 off, in both directions (prediction and its transpose).

Method (that of tools/f64_time.py): device events around `calls` back-to-back products, minimum (and maximum) over
`rounds` rounds, the variants alternating round by round in one process on the same points, after a warm-up of each
(lattices, tables, workspaces, code objects).  Peak memory per variant: torch.cuda.max_memory_allocated of one warm product
above what was resident before it, and plx_device_bytes of the lattices the variant's operators use.

    python tools/rows_f64_time.py [--out profiles/rows_f64_measured.md] [--rounds 7] [--calls 20] [--columns 1 11 101]

Shape: that of profiles/rows_measured.md -- N = 1e6 training rows, 2.5e5 held-out rows, d = 8, RBF order 1, lengthscale
0.6931, everything in double.  Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from tools.f64_time import timed  # noqa: E402

RLL = plx.RectangularLazyLattice


def run(native, fn):
    RLL.native_rows_f64 = native
    return fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 11, 101])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--n-star", type=int, default=250_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rows_f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda", 0)
    n, ns, d = args.n, args.n_star, 8
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=g, dtype=torch.float64).to(dev)
    xs = torch.randn(ns, d, generator=g, dtype=torch.float64).to(dev)
    k = plx.RBFLattice(order=1, ard_num_dims=d).double().to(dev)      # lengthscale softplus(0) = 0.6931
    for prm in k.parameters():
        prm.requires_grad_(False)
    keep = (RLL.native_rows_f64, RLL.native_min_columns)
    RLL.native_min_columns = 1                       # the C ABI serves every width; the gate is what is being decided
    lines = ["| columns | direction | native ms min / max | padded ms min / max | native / padded | native torch peak MB | "
             "padded torch peak MB | native lattice MB | padded lattice MB | kernels |", "|---|---|---|---|---|---|---|---|---|---|"]
    cache = plx.lattice_cache()
    try:
        with torch.no_grad():
            for c in args.columns:
                V = torch.randn(n, c, generator=g, dtype=torch.float64).to(dev)
                G = torch.randn(ns, c, generator=g, dtype=torch.float64).to(dev)
                cache.clear()
                torch.cuda.empty_cache()
                R = {True: k(xs, x), False: k(xs, x)}          # one operator per route: each keeps its own stacked points
                Rt = {r: R[r].t() for r in R}
                legs = {("prediction", r): (lambda r=r: run(r, lambda: R[r].matmul(V))) for r in (True, False)}
                legs.update({("transpose", r): (lambda r=r: run(r, lambda: Rt[r].matmul(G))) for r in (True, False)})
                lat_mb, peak = {}, {}
                def warm(route):
                    for key, fn in legs.items():
                        if key[1] == route:
                            for _ in range(3):
                                fn()
                    torch.cuda.synchronize()
                    return sum(e[0].device_bytes for e in cache._entries.values()) / 1e6

                for route in (False, True):                     # each route alone first: the lattices it needs, in MB
                    cache.clear()
                    lat_mb[route] = warm(route)
                warm(False)                                     # ... then both warm side by side
                same = all(torch.equal(legs[(dn, True)](), legs[(dn, False)]()) for dn in ("prediction", "transpose"))
                for key, fn in legs.items():
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    fn()
                    torch.cuda.synchronize()
                    peak[key] = (torch.cuda.max_memory_allocated() - base) / 1e6
                lo = {key: float("inf") for key in legs}
                hi = {key: 0.0 for key in legs}
                for _ in range(args.rounds):
                    for key, fn in legs.items():                # alternating: every round times every variant once
                        t = timed(fn, args.calls)
                        lo[key], hi[key] = min(lo[key], t), max(hi[key], t)
                lat = cache.get(R[True]._stacked_points(), k.dkernel_fn.get_coeffs())
                kn = lat.rows_f64_kernels()
                for dn in ("prediction", "transpose"):
                    a, b = (dn, True), (dn, False)
                    lines.append(f"| {c} | {dn} | {lo[a]:.3f} / {hi[a]:.3f} | {lo[b]:.3f} / {hi[b]:.3f} | {lo[a] / lo[b]:.2f} | "
                                 f"{peak[a]:.0f} | {peak[b]:.0f} | {lat_mb[True]:.0f} | {lat_mb[False]:.0f} | "
                                 f"{'+'.join(kn['splat'] + kn['slice'])}; equal values: {same} |")
                    print(lines[-1], flush=True)
                del V, G, R, Rt, legs
    finally:
        RLL.native_rows_f64, RLL.native_min_columns = keep
        cache.clear()
    text = (f"device: {torch.cuda.get_device_name(0)}; N = {n} + {ns}, d = {d}, order 1, float64; minimum / maximum of "
            f"{args.rounds} rounds of {args.calls} back-to-back products, device events, the four variants alternating\n\n"
            + "\n".join(lines) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
