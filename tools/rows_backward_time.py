"""Time the fp32 position gradient of the rectangular product K(xin, xout) V: the native route (two one-sided
plx_apply_backward_rows calls of half the padded width, RectangularLazyLattice.native_rows_grad = True) against the padded
route that runs with the switch off (one square position gradient over the zero-padded stack: plx_apply_backward where the
shape is fusable, else the stored stack, plx_apply and the contraction).  The padded route is the baseline.

What is timed is what a caller runs: (op._matmul(V) * W).sum().backward() in float32 with xin and xout both wanting a
gradient, i.e. the forward product, the lattice builds of the fresh stacked tensor (forward taps and derivative taps; both
routes pay them) and the position gradient.  V wants no gradient (the gradient of a predictive mean with respect to inputs).

Method (that of tools/rows_backward_f64_time.py): device events around `calls` back-to-back steps, the minimum over `rounds`
rounds, the two routes alternating round by round in one process on the same points, after a warm-up of each.  Next to the
minimum the spread (max - min over the rounds, as a share of the minimum): a difference inside it says nothing.  Workspace:
plx_device_bytes summed over the lattices the route left in the cache after one step from an empty cache, and
torch.cuda.max_memory_allocated over one warm step above what was allocated before it.  Every (shape, L) runs in a child
process of its own under a time limit; a child that fails or runs out of time ends the run.

    python tools/rows_backward_time.py [--out profiles/rows_backward_measured.md] [--rounds 7] [--calls 3] [--limit 240]

Shapes: N = 1e6 + 2.5e5, d = 8, RBF order 1 (L = 1: 18 stacked columns, not fusable, the padded route stores the stack;
L = 11: fusable); the config-5 stand-in (MaternLattice nu = 1.5, order 3, N = 10,623 + 2,656, d = 18); L in {1, 11}; both
directions (the operator and its transpose).  Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import subprocess
import sys

HEADER = ["| shape | L | direction | native ms (spread) | padded ms (spread) | native / padded | lattice MB native / padded | "
          "torch peak MB native / padded | max rel. difference of the position gradients | native kernels | padded kernels |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
SHAPES = [("N = 1e6 + 2.5e5, d = 8, RBF order 1", 1_000_000, 250_000, 8),
          ("N = 10,623 + 2,656, d = 18, Matern-3/2 order 3 (config-5 stand-in)", 10_623, 2_656, 18)]


def child(shape, c, rounds, calls):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import simplex_gp_amd as plx
    from tools.backward_f64_time import timed

    if not torch.cuda.is_available():
        raise SystemExit("rows_backward_time.py needs a GPU: a CPU run says nothing about these kernels")
    RLL = plx.RectangularLazyLattice
    dev = torch.device("cuda", 0)
    name, n, ns, d = SHAPES[shape]
    kern = plx.RBFLattice(order=1, ard_num_dims=d) if shape == 0 else plx.MaternLattice(nu=1.5, order=3, ard_num_dims=d)
    dk = kern.dkernel_fn
    gen = torch.Generator().manual_seed(1234)
    scale = 1.0 / 0.6931
    xout = (torch.randn(n, d, generator=gen) * scale).to(dev).requires_grad_(True)
    xin = (torch.randn(ns, d, generator=gen) * scale).to(dev).requires_grad_(True)
    leaves = (xin, xout)
    cache = plx.lattice_cache()

    def step(native, op, V, W):
        RLL.native_rows_grad = native
        for t in leaves:
            t.grad = None
        (op._matmul(V) * W).sum().backward()
        return [t.grad for t in leaves]

    keep = RLL.native_rows_grad
    try:
        data = {"prediction": (RLL(xin, xout, dk), n, ns), "transpose": (RLL(xin, xout, dk)._transpose_nonbatch(), ns, n)}
        for direction, (op, rows_v, rows_w) in data.items():
            V = torch.randn(rows_v, c, generator=gen).to(dev)
            W = torch.randn(rows_w, c, generator=gen).to(dev)
            runs = {"native": (lambda: step(True, op, V, W)), "padded": (lambda: step(False, op, V, W))}
            lat_mb, peak, grads, kn = {}, {}, {}, {}
            for r, fn in runs.items():
                cache.clear()
                torch.cuda.empty_cache()
                grads[r] = [t.clone() for t in fn()]
                torch.cuda.synchronize()
                lat_mb[r] = sum(e[0].device_bytes for e in cache._entries.values()) / 1e6
                names = set()
                for e in cache._entries.values():
                    fam = e[0].rows_kernels() if r == "native" else e[0].stage_kernels()
                    names.update(x for x in fam["splat"] + fam["slice"] if r == "padded" or "backward" in x)
                kn[r] = "+".join(sorted(names))
                fn()                                            # warm: code objects, allocator
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                peak[r] = (torch.cuda.max_memory_allocated() - base) / 1e6
            assert all(bool(torch.isfinite(t).all()) for r in grads for t in grads[r]), "a position gradient is not finite"
            # relative to the largest entry of the padded gradient; a gradient that vanishes altogether compares absolutely
            diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads["native"], grads["padded"]))
            del grads
            times = {r: [] for r in runs}
            for _ in range(rounds):
                for r, fn in runs.items():                      # alternating: every round times every route once
                    times[r].append(timed(fn, calls))
            best = {r: min(v) for r, v in times.items()}
            cell = lambda r: f"{best[r]:.3f} ({(max(times[r]) - best[r]) / best[r] * 100:.1f} %)"      # noqa: E731
            print(f"ROW | {name} | {c} | {direction} | {cell('native')} | {cell('padded')} | "
                  f"{best['native'] / best['padded']:.2f} | {lat_mb['native']:.0f} / {lat_mb['padded']:.0f} | "
                  f"{peak['native']:.0f} / {peak['padded']:.0f} | {diff:.1e} | {kn['native']} | {kn['padded']} |", flush=True)
            del V, W, runs
        print("DEVICE " + torch.cuda.get_device_name(0), flush=True)
    finally:
        RLL.native_rows_grad = keep
        cache.clear()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 11])
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--child", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.rounds, args.calls)
    lines, device = list(HEADER), "?"
    for shape in range(len(SHAPES)):
        for c in args.columns:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(shape), str(c), "--rounds", str(args.rounds),
                   "--calls", str(args.calls)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)     # the child is killed at the limit
            if done.returncode != 0:
                raise SystemExit(f"shape {shape}, L = {c}: the child ended with {done.returncode}\n{done.stdout}\n{done.stderr}")
            for line in done.stdout.splitlines():
                if line.startswith("ROW "):
                    lines.append(line[4:])
                    print(line[4:], flush=True)
                elif line.startswith("DEVICE "):
                    device = line[7:]
    text = (f"device: {device}; float32; one step = (op._matmul(V) * W).sum().backward() with xin and xout wanting a gradient "
            f"(forward product, both lattice builds of the fresh stacked tensor, position gradient); minimum of {args.rounds} "
            f"rounds of {args.calls} steps, device events, the two routes alternating in one process per (shape, L); spread = "
            "(max - min) / min over the rounds; lattice MB = plx_device_bytes of the lattices in the cache after one step from an "
            "empty cache (the workspace included); torch peak = torch.cuda.max_memory_allocated over one warm step minus what was "
            "allocated before it\n\n" + "\n".join(lines) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
