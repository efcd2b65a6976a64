"""Time the true diagonal of the lattice operator: plx_diag and plx_diag_f64 (one launch each, csrc/plx_diag_kernels.h) next
to one single-column product of the same precision on the same lattice (plx_apply / plx_apply_f64: the only other way to the
same numbers is n of them) and next to the lattice build the diagonal is computed once for.

Method (that of tools/sym_f64_time.py): device events around `calls` back-to-back calls, the minimum over `rounds` rounds,
the routes alternating round by round in one process on one lattice, after a warm-up of all of them.  Next to the minimum
the spread (max - min over the rounds, as a share of the minimum) is recorded: a difference inside it says nothing.  The
build is timed one call per round, device events around Lattice.build (it reads a few counts back, so the time includes
those waits).

Also the iteration counts of the yardstick solve (a LatticeGP(RBFLattice) on the Gaussian cloud n = 2000, d = 3, three
right-hand sides, noise 1.0 and 0.1, the rank-100 native preconditioner, tol 1e-6 in fp32 and 1e-11 in float64) with the
preconditioner's true_diag off and on: the evidence a change of that default would need.

    python tools/diag_time.py [--out profiles/diag_time.md] [--rounds 5] [--calls 20]

Shapes: N = 1e6, d = 8, order 1; N = 2e4, d = 4, order 1; the config-5 stand-in (MaternLattice nu = 1.5, order 3,
N = 10,623, d = 18).  Needs a GPU.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import solvers  # noqa: E402


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def shapes():
    rbf1 = plx.DiscretizedKernelFN(plx.rbf, 1).get_coeffs().numpy()
    taps5 = plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18).dkernel_fn.get_coeffs().numpy()
    return [("N = 1e6, d = 8, order 1", 1_000_000, 8, rbf1), ("N = 2e4, d = 4, order 1", 20_000, 4, rbf1),
            ("N = 10,623, d = 18, order 3 (config-5 stand-in)", 10_623, 18, taps5)]


def cell(ts):
    best = min(ts)
    return f"{best:.4f} ({(max(ts) - best) / best * 100:.1f} %)"


def measure(rounds, calls):
    dev = torch.device("cuda", 0)
    lines = ["| shape | m | diagonal: min / mean / max | plx_diag ms (spread) | plx_apply, 1 column ms (spread) | "
             "plx_diag_f64 ms (spread) | plx_apply_f64, 1 column ms (spread) | build ms (spread) | "
             "max abs(fp32 - float64) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, n, d, taps in shapes():
        gen = torch.Generator().manual_seed(1234)
        x = torch.randn(n, d, generator=gen).to(dev)
        lat = plx.Lattice(dev).build(x, taps)
        v32 = torch.randn(n, 1, generator=gen).to(dev)
        v64 = v32.double()
        o32, o64 = torch.empty_like(v32), torch.empty_like(v64)
        d32 = torch.empty(n, dtype=torch.float32, device=dev)
        d64 = torch.empty(n, dtype=torch.float64, device=dev)
        runs = {"diag": lambda: lat.diag(torch.float32, out=d32), "apply": lambda: lat.apply(v32, out=o32),
                "diag64": lambda: lat.diag(torch.float64, out=d64), "apply64": lambda: lat.apply(v64, out=o64)}
        for fn in runs.values():                                  # warm-up: workspaces grown, tables built
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        times["build"] = []
        for _ in range(rounds):
            for k, fn in runs.items():                            # alternating: every round times every route once
                times[k].append(timed(fn, calls))
        for _ in range(rounds):
            times["build"].append(timed(lambda: lat.build(x, taps), 1))
        lat.diag(torch.float32, out=d32)
        lat.diag(torch.float64, out=d64)
        gap = float((d32.double() - d64).abs().max())
        lines.append(f"| {name} | {lat.m} | {float(d64.min()):.3f} / {float(d64.mean()):.3f} / {float(d64.max()):.3f} | "
                     f"{cell(times['diag'])} | {cell(times['apply'])} | {cell(times['diag64'])} | {cell(times['apply64'])} | "
                     f"{cell(times['build'])} | {gap:.2e} |")
        lat.close()
        del x, v32, v64, o32, o64, d32, d64
        torch.cuda.empty_cache()
    return lines


def solve_counts():
    """Preconditioned CG iterations of the yardstick solve with the factor started from the declared and the true diagonal."""
    n, d, rank = 2000, 3, 100
    x64 = torch.randn(n, d, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    lines = ["| precision | noise | tol | iterations, true_diag off | iterations, true_diag on | worst residual off | "
             "worst residual on |", "|---|---|---|---|---|---|---|"]
    for dtype, tol in ((torch.float32, 1e-6), (torch.float64, 1e-11)):
        for noise in (1.0, 0.1):
            model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).to(dtype).cuda()
            x, rhs = x64.to(dtype).cuda(), B.to(dtype).cuda()
            with torch.no_grad():
                model.raw_noise.fill_(math.log(math.expm1(noise - model.min_noise)))
                K = model.kernel(x, x)
                off = model.preconditioner(x, rank, K=K)
                cls = type(off)
                kw = {} if cls is solvers.LatticePreconditioner64 else {"factor_dtype": torch.float16}
                on = cls(off.lat, model.outputscale, model.noise, rank, true_diag=True, **kw)
                row = []
                for pre in (off, on):
                    _, info = model.khat_solve(x, rhs, K=K, tol=tol, max_iter=500, precond=pre)
                    row.append((int(info["iterations"]), float(info["residual"].max())))
            lines.append(f"| {str(dtype).split('.')[-1]} | {noise} | {tol:g} | {row[0][0]} | {row[1][0]} | {row[0][1]:.2e} | "
                         f"{row[1][1]:.2e} |")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diag_time.py needs a GPU: a CPU run says nothing about these kernels")
    text = (f"device: {torch.cuda.get_device_name(0)}; minimum of {args.rounds} rounds of {args.calls} back-to-back calls, "
            "device events, the routes alternating; spread = (max - min) / min over the rounds\n\n"
            + "\n".join(measure(args.rounds, args.calls)) + "\n\n"
            "Yardstick solve (n = 2000, d = 3, rank-100 preconditioner, three right-hand sides): preconditioned CG iterations\n\n"
            + "\n".join(solve_counts()) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
