"""Time the float64 position gradient: the native call (plx_apply_backward_f64) next to the torch route around the native fp64
product (LatticeFilterGeneral.backward with fused_backward_f64 = False).

Method (that of tools/cg_f64_time.py): device events around `calls` back-to-back gradients, the minimum over `rounds` rounds,
the two routes alternating round by round in one process on one lattice, after a warm-up of both.  Next to the minimum the
spread (max - min over the rounds, as a share of the minimum) is recorded: a difference inside it says nothing.  Peak memory:
torch.cuda.max_memory_allocated over one gradient of each route, minus what was allocated before it (the torch route's
temporaries are torch tensors; the native route's workspace belongs to the lattice, so Lattice.device_bytes is printed too).

Both routes compute (grad_x, grad_src) from the same (g, src, x) on the derivative-tap lattice of x, L = 11 columns:
    native   Lattice.apply_backward(g, src, x) in float64
    torch    two outer products, torch.cat into the n x 2L(1+d) stack, Lattice.apply of it, split, four broadcast products
             and a sum(-2): the statements of LatticeFilterGeneral.backward's last branch

    python tools/backward_f64_time.py [--out profiles/backward_f64_time.md] [--rounds 7] [--calls 5]

Shapes: N = 1e6, d = 8, order 1 (the training shape); N = 2e4, d = 4, order 1; the config-5 stand-in (MaternLattice nu = 1.5,
order 3, N = 10,623, d = 18).  Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402

L = 11


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_route(lat, g, src, ref):
    """The last branch of LatticeFilterGeneral.backward, statement by statement, on a lattice at hand."""
    d = ref.shape[-1]
    gx = (g[..., None] * ref[..., None, :])
    sx = (src[..., None] * ref[..., None, :])
    stacked = torch.cat([g, gx.reshape(gx.shape[:-2] + (L * d,)), src, sx.reshape(sx.shape[:-2] + (L * d,))], dim=-1)
    filtered = lat.apply(stacked.contiguous())
    wg, wgx, ws, wsx = torch.split(filtered, [L, L * d, L, L * d], dim=-1)
    wgx = wgx.reshape(-1, L, d)
    wsx = wsx.reshape(-1, L, d)
    grad_reference = -2 * (sx * wg[..., None] - src[..., None] * wgx + gx * ws[..., None] - g[..., None] * wsx).sum(-2)
    return grad_reference, wg


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("backward_f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda", 0)
    rbf1 = plx.DiscretizedKernelFN(plx.rbf, 1).get_deriv_coeffs().numpy()
    taps5 = plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18).dkernel_fn.get_deriv_coeffs().numpy()
    shapes = [("N = 1e6, d = 8, order 1", 1_000_000, 8, rbf1), ("N = 2e4, d = 4, order 1", 20_000, 4, rbf1),
              ("N = 10,623, d = 18, order 3 (config-5 stand-in)", 10_623, 18, taps5)]
    lines = ["| shape | m | columns | native ms (spread) | torch ms (spread) | torch / native | native peak MiB (+ lattice workspace) "
             "| torch peak MiB (+ lattice workspace) | max rel. difference of grad_x |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, n, d, taps in shapes:
        gen = torch.Generator().manual_seed(1234)
        x = torch.randn(n, d, generator=gen, dtype=torch.float64).to(dev)
        g = torch.randn(n, L, generator=gen, dtype=torch.float64).to(dev)
        src = torch.randn(n, L, generator=gen, dtype=torch.float64).to(dev)
        lat = plx.Lattice(dev).build(x.float(), taps)
        runs = {"native": lambda: lat.apply_backward(g, src, x), "torch": lambda: torch_route(lat, g, src, x)}
        bytes0 = lat.device_bytes
        # peak memory first, native before torch: the lattice's float64 workspace grows once, with the first of them
        peaks, work = {}, {}
        for k, fn in runs.items():
            peaks[k] = peak(fn)
            work[k] = (lat.device_bytes - bytes0) / 2 ** 20
        a, b = runs["native"]()[0], runs["torch"]()[0]
        diff = float(((a - b).abs().max() / b.abs().max()))
        del a, b
        for fn in runs.values():                                  # warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():                            # alternating: every round times both routes once
                times[k].append(timed(fn, args.calls))
        best = {k: min(v) for k, v in times.items()}
        cell = lambda k: f"{best[k]:.3f} ({(max(times[k]) - best[k]) / best[k] * 100:.1f} %)"      # noqa: E731
        lines.append(f"| {name} | {lat.m} | {2 * L * (1 + d)} | {cell('native')} | {cell('torch')} | "
                     f"{best['torch'] / best['native']:.2f} | {peaks['native']:.0f} (+ {work['native']:.0f}) | "
                     f"{peaks['torch']:.0f} (+ {work['torch']:.0f}) | {diff:.1e} |")
        print(lines[-1], flush=True)
        lat.close()
        del x, g, src
        torch.cuda.empty_cache()
    text = (f"device: {torch.cuda.get_device_name(0)}; L = {L} columns of doubles; minimum of {args.rounds} rounds of {args.calls} "
            "gradients, device events, the routes alternating; spread = (max - min) / min over the rounds; peak = "
            "torch.cuda.max_memory_allocated over one gradient minus what was allocated before it, (+ growth of "
            "Lattice.device_bytes up to and including that route's first gradient: the native route runs first and grows the "
            "float64 workspace both routes use)\n\n" + "\n".join(lines) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
