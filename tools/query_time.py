"""Time the queries at points that are not the build's: plx_locate (locate_kernel, csrc/plx_build.hip) and plx_slice_at
(csrc/plx_query_kernels.h) at 1 / 16 / 101 columns, for n* = 1, 1e4, 1e5 held-out points, and PredictionCache.predict by
both routes on one cache -- route="stacked" (a lattice over [x*; X] built per batch, the 1 + t columns splatted and
blurred on it: code the query route does not touch, hence the yardstick) against route="query" (the training lattice's
blurred columns sliced at x*).

Method (that of tools/diag_time.py): device events around `calls` back-to-back calls, the MEDIAN over `rounds` rounds, the
routes alternating round by round in one process, after a warm-up of all of them; next to the median the spread (max - min
over the rounds, as a share of the median): a difference inside it says nothing.  A predict is timed one call per round (it
builds a lattice and synchronises on its counts on the stacked route).

    python tools/query_time.py [--out profiles/query_time.md] [--rounds 5] [--calls 20] [--no-predict]

Shapes: N = 1e6, d = 8, order 1; the config-5 stand-in (MaternLattice nu = 1.5, order 3, N = 10,623, d = 18).  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import solvers, training  # noqa: E402

NSTAR = (1, 10_000, 100_000)
COLUMNS = (1, 16, 101)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def cell(ts):
    med = statistics.median(ts)
    return f"{med:.4f} ({(max(ts) - min(ts)) / med * 100:.1f} %)"


def shapes():
    rbf1 = plx.DiscretizedKernelFN(plx.rbf, 1).get_coeffs().numpy()
    taps5 = plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18).dkernel_fn.get_coeffs().numpy()
    return [("N = 1e6, d = 8, order 1", 1_000_000, 8, rbf1),
            ("N = 10,623, d = 18, order 3 (config-5 stand-in)", 10_623, 18, taps5)]


def measure_kernels(rounds, calls):
    dev = torch.device("cuda", 0)
    lines = ["| shape | m | n* | found share | locate ms (spread) | " +
             " | ".join(f"slice_at, {c} columns ms (spread)" for c in COLUMNS) + " |",
             "|---|---|---|---|---|" + "---|" * len(COLUMNS)]
    for name, n, d, taps in shapes():
        gen = torch.Generator().manual_seed(1234)
        x = torch.randn(n, d, generator=gen).to(dev)
        lat = plx.Lattice(dev).build(x, taps)
        blurred = {c: lat.blurred(torch.randn(n, c, generator=gen).to(dev)) for c in COLUMNS}
        for ns in NSTAR:
            xs = torch.randn(ns, d, generator=gen).to(dev)
            q = lat.locate(xs)
            share = float((q.vid >= 0).float().mean())
            outs = {c: torch.empty(ns, c, device=dev) for c in COLUMNS}
            runs = {"locate": lambda: lat.locate(xs)}
            for c in COLUMNS:
                runs[c] = (lambda c=c: lat.slice_at(blurred[c][0], q, out=outs[c], vd=c))
            for fn in runs.values():
                fn()
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(rounds):
                for k, fn in runs.items():                        # alternating: every round times every call once
                    times[k].append(timed(fn, calls))
            lines.append(f"| {name} | {lat.m} | {ns} | {share:.3f} | {cell(times['locate'])} | " +
                         " | ".join(cell(times[c]) for c in COLUMNS) + " |")
        lat.close()
        del x, blurred
        torch.cuda.empty_cache()
    return lines


def measure_predict(rounds):
    """One PredictionCache (rank-100 preconditioner, 100 Lanczos steps: 1 + 100 columns) per shape, both routes on it."""
    dev = torch.device("cuda", 0)
    lines = ["| shape | n* | predict, stacked ms (spread) | predict, query ms (spread) | stacked / query | "
             "mass of the batch: min / median / mean |", "|---|---|---|---|---|---|"]
    for name, n, d, kernel in (("N = 1e6, d = 8, RBF order 1", 1_000_000, 8, plx.RBFLattice(order=1, ard_num_dims=8)),
                               ("N = 10,623, d = 18, Matern-3/2 order 3 (config-5 stand-in)", 10_623, 18,
                                plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18))):
        gen = torch.Generator().manual_seed(99)
        x = torch.randn(n, d, generator=gen).to(dev)
        y = (torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=gen).to(dev))
        model = solvers.LatticeGP(kernel).to(dev)
        cache = training.PredictionCache(model, x, y, lanc_iter=100, pre_size=100)
        for ns in NSTAR:
            xs = torch.randn(ns, d, generator=gen).to(dev)
            runs = {r: (lambda r=r: cache.predict(xs, route=r)) for r in ("stacked", "query")}
            for fn in runs.values():
                fn()
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(rounds):
                for k, fn in runs.items():
                    times[k].append(timed(fn, 1))
            cache.predict(xs, route="query")
            mass = cache.last_query_mass
            ratio = statistics.median(times["stacked"]) / statistics.median(times["query"])
            lines.append(f"| {name} | {ns} | {cell(times['stacked'])} | {cell(times['query'])} | {ratio:.1f} | "
                         f"{float(mass.min()):.3f} / {float(mass.median()):.3f} / {float(mass.mean()):.3f} |")
        del cache, model, x, y
        plx.lattice_cache().clear()
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-predict", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_time.py needs a GPU: a CPU run says nothing about these kernels")
    text = (f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of {args.calls} back-to-back calls, "
            "device events, the calls alternating; spread = (max - min) / median over the rounds; held-out queries: a fresh "
            "draw of the cloud\n\n" + "\n".join(measure_kernels(args.rounds, args.calls)) + "\n")
    if not args.no_predict:
        text += ("\nPredictionCache.predict (1 + 100 columns), one call per round, both routes on one cache\n\n"
                 + "\n".join(measure_predict(args.rounds)) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
