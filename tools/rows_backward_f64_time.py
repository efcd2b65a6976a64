"""Time the float64 position gradient of the rectangular product K(xin, xout) V: the native route (two one-sided
plx_apply_backward_rows_f64 calls of half the padded width, RectangularLazyLattice.native_rows_grad_f64 = True) against the
padded route that runs with the switch off (one square position gradient over the zero-padded stack).

What is timed is what a caller runs: (op._matmul(V) * W).sum().backward() in double with xin and xout both wanting a
gradient, i.e. the forward product, the lattice builds of the fresh stacked tensor (forward taps and derivative taps; both
routes pay them) and the position gradient.  V wants no gradient (the gradient of a predictive mean with respect to inputs).
Three routes: native; padded (the default: LatticeFilterGeneral.fused_backward_f64 = False, the torch stack and contraction
around the native fp64 product); padded-fused (fused_backward_f64 = True: plx_apply_backward_f64 over all n rows).

Method (that of tools/rows_f64_time.py and tools/backward_f64_time.py): device events around `calls` back-to-back steps, the
minimum over `rounds` rounds, the routes alternating round by round in one process on the same points, after a warm-up of
each.  Next to the minimum the spread (max - min over the rounds, as a share of the minimum): a difference inside it says
nothing.  Workspace: plx_device_bytes summed over the lattices the route left in the cache after one step from an empty
cache, and torch.cuda.max_memory_allocated over one warm step above what was allocated before it.

    python tools/rows_backward_f64_time.py [--out profiles/rows_backward_f64_measured.md] [--rounds 7] [--calls 3]

Shapes: N = 1e6 + 2.5e5, d = 8, RBF order 1; the config-5 stand-in (MaternLattice nu = 1.5, order 3, N = 10,623 + 2,656,
d = 18); L in {1, 11}; both directions (the operator and its transpose).  Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from tools.backward_f64_time import timed  # noqa: E402

RLL, LFG = plx.RectangularLazyLattice, plx.LatticeFilterGeneral
ROUTES = {"native": (True, False), "padded": (False, False), "padded-fused": (False, True)}


def step(route, op, V, W, leaves):
    RLL.native_rows_grad_f64, LFG.fused_backward_f64 = ROUTES[route]
    for t in leaves:
        t.grad = None
    (op._matmul(V) * W).sum().backward()
    return [t.grad for t in leaves]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 11])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rows_backward_f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda", 0)
    shapes = [("N = 1e6 + 2.5e5, d = 8, RBF order 1", 1_000_000, 250_000, 8, plx.RBFLattice(order=1, ard_num_dims=8)),
              ("N = 10,623 + 2,656, d = 18, Matern-3/2 order 3 (config-5 stand-in)", 10_623, 2_656, 18,
               plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18))]
    lines = ["| shape | L | direction | native ms (spread) | padded ms (spread) | padded-fused ms (spread) | native / padded | "
             "native / padded-fused | lattice MB native / padded / padded-fused | torch peak MB native / padded / padded-fused | "
             "max rel. difference of the position gradients | kernels |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    keep = (RLL.native_rows_grad_f64, LFG.fused_backward_f64)
    cache = plx.lattice_cache()
    try:
        for name, n, ns, d, kern in shapes:
            dk = kern.dkernel_fn
            gen = torch.Generator().manual_seed(1234)
            scale = 1.0 / 0.6931
            xout = (torch.randn(n, d, generator=gen, dtype=torch.float64) * scale).to(dev).requires_grad_(True)
            xin = (torch.randn(ns, d, generator=gen, dtype=torch.float64) * scale).to(dev).requires_grad_(True)
            leaves = (xin, xout)
            for c in args.columns:
                data = {"prediction": (RLL(xin, xout, dk), n, ns), "transpose": (RLL(xin, xout, dk)._transpose_nonbatch(), ns, n)}
                for direction, (op, rows_v, rows_w) in data.items():
                    V = torch.randn(rows_v, c, generator=gen, dtype=torch.float64).to(dev)
                    W = torch.randn(rows_w, c, generator=gen, dtype=torch.float64).to(dev)
                    runs = {r: (lambda r=r: step(r, op, V, W, leaves)) for r in ROUTES}
                    lat_mb, peak, grads, kn = {}, {}, {}, ""
                    for r, fn in runs.items():
                        cache.clear()
                        torch.cuda.empty_cache()
                        grads[r] = [t.clone() for t in fn()]
                        torch.cuda.synchronize()
                        lat_mb[r] = sum(e[0].device_bytes for e in cache._entries.values()) / 1e6
                        if r == "native":
                            names = set()
                            for e in cache._entries.values():
                                fam = e[0].rows_f64_kernels()
                                names.update(x for x in fam["splat"] + fam["slice"] if "backward" in x)
                            kn = "+".join(sorted(names))
                        fn()                                            # warm: code objects, allocator
                        torch.cuda.synchronize()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        fn()
                        torch.cuda.synchronize()
                        peak[r] = (torch.cuda.max_memory_allocated() - base) / 1e6
                    diff = max(float((a - b).abs().max() / b.abs().max())
                               for r in ("padded", "padded-fused") for a, b in zip(grads["native"], grads[r]))
                    del grads
                    times = {r: [] for r in runs}
                    for _ in range(args.rounds):
                        for r, fn in runs.items():                      # alternating: every round times every route once
                            times[r].append(timed(fn, args.calls))
                    best = {r: min(v) for r, v in times.items()}
                    cell = lambda r: f"{best[r]:.3f} ({(max(times[r]) - best[r]) / best[r] * 100:.1f} %)"      # noqa: E731
                    three = lambda t: " / ".join(f"{t[r]:.0f}" for r in ROUTES)                                # noqa: E731
                    lines.append(f"| {name} | {c} | {direction} | {cell('native')} | {cell('padded')} | {cell('padded-fused')} | "
                                 f"{best['native'] / best['padded']:.2f} | {best['native'] / best['padded-fused']:.2f} | "
                                 f"{three(lat_mb)} | {three(peak)} | {diff:.1e} | {kn} |")
                    print(lines[-1], flush=True)
                    del V, W, runs
            xin.grad = xout.grad = None
            del xin, xout, leaves, data
            cache.clear()
            torch.cuda.empty_cache()
    finally:
        RLL.native_rows_grad_f64, LFG.fused_backward_f64 = keep
        cache.clear()
    text = (f"device: {torch.cuda.get_device_name(0)}; float64; one step = (op._matmul(V) * W).sum().backward() with xin and xout "
            f"wanting a gradient (forward product, both lattice builds of the fresh stacked tensor, position gradient); minimum of "
            f"{args.rounds} rounds of {args.calls} steps, device events, the three routes alternating; spread = (max - min) / min "
            "over the rounds; lattice MB = plx_device_bytes of the lattices in the cache after one step from an empty cache (the "
            "float64 workspace included); torch peak = torch.cuda.max_memory_allocated over one warm step minus what was "
            "allocated before it\n\n" + "\n".join(lines) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
