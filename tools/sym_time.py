"""Time the symmetrised fp32 product: plx_apply_sym (one splat, d + 1 launches of blur_dual_kernel that advance both blur
chains, one slice) next to one plx_apply (what a solve on K itself pays per iteration) and next to plx_apply + plx_apply_t
back to back (the two full products it replaces).

Unlike the float64 product, the plain fp32 blur picks among ten kernel families and on cache-resident lattices runs two
axes per launch; plx_apply_sym and plx_apply_t run one general family, one axis per launch.  So this is NOT the float64
comparison over again: the table records which family the plain blur took.

Method (that of tools/sym_f64_time.py, with medians): device events around a window of back-to-back products, the median
over `rounds` rounds, the routes alternating round by round in one process on one lattice, after a warm-up of all of them.
A window holds at least `calls` products and at least `window-ms` of work (a product of 0.03 ms timed 20 at a time measures
the scheduler: 35..80 % spread), the count fixed per route from a trial after the warm-up.
Next to the median the spread (max - min over the rounds, as a share of the median) is recorded: a difference inside it
says nothing.  The outputs of the timed routes are compared once per shape (K_s v against (K v + K^T v) / 2, rel-L2).

    python tools/sym_time.py [--out profiles/sym_time.md] [--rounds 9] [--calls 20] [--window-ms 50]

Shapes: N = 1e6, d = 8, order 1; N = 2e4, d = 4, order 1; the config-5 stand-in (MaternLattice nu = 1.5, order 3,
N = 10,623, d = 18); widths 1, 4 and 16.  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402

WIDTHS = (1, 4, 16)


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


def measure(rounds, calls, window_ms):
    """[(shape name, m, vd, plain blur family, {route: [ms per round]}, rel-L2 of K_s v against (K v + K^T v) / 2)]"""
    dev = torch.device("cuda", 0)
    rows = []
    for name, n, d, taps in shapes():
        gen = torch.Generator().manual_seed(1234)
        x = torch.randn(n, d, generator=gen).to(dev)
        lat = plx.Lattice(dev).build(x, taps)
        for vd in WIDTHS:
            v = torch.randn(n, vd, generator=gen).to(dev)
            o1, o2 = torch.empty_like(v), torch.empty_like(v)
            runs = {"plain": lambda: lat.apply(v, out=o1), "sym": lambda: lat.apply_sym_f32(v, out=o1),
                    "pair": lambda: (lat.apply(v, out=o1), lat.apply_t_f32(v, out=o2))}
            for fn in runs.values():                                  # warm-up: workspaces grown, tables built
                fn()
                fn()
            torch.cuda.synchronize()
            family = "+".join(lat.stage_kernels()["blur_axis"])
            mean = 0.5 * (lat.apply(v).double() + lat.apply_t_f32(v).double())
            gap = float((lat.apply_sym_f32(v).double() - mean).norm() / mean.norm())
            count = {k: max(calls, int(window_ms / max(timed(fn, calls), 1e-4)) + 1) for k, fn in runs.items()}
            times = {k: [] for k in runs}
            for _ in range(rounds):
                for k, fn in runs.items():                            # alternating: every round times every route once
                    times[k].append(timed(fn, count[k]))
            rows.append((name, lat.m, vd, family, times, gap))
            del v, o1, o2, mean
        lat.close()
        del x
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=50.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sym_time.py needs a GPU: a CPU run says nothing about these kernels")
    rows = measure(args.rounds, args.calls, args.window_ms)

    def cell(ts):
        med = statistics.median(ts)
        return f"{med:.4f} ({(max(ts) - min(ts)) / med * 100:.1f} %)"

    lines = ["| shape | m | columns | plain blur family | apply_sym ms (spread) | apply + apply_t ms (spread) | "
             "one apply ms (spread) | sym / (apply + apply_t) | sym / one apply | rel-L2 sym vs (K + K^T) / 2 |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, m, vd, family, t, gap in rows:
        sym, pair, plain = (statistics.median(t[k]) for k in ("sym", "pair", "plain"))
        lines.append(f"| {name} | {m} | {vd} | `{family}` | {cell(t['sym'])} | {cell(t['pair'])} | {cell(t['plain'])} | "
                     f"{sym / pair:.2f} | {sym / plain:.2f} | {gap:.1e} |")
    text = (f"device: {torch.cuda.get_device_name(0)}; float32 right-hand sides; median of {args.rounds} rounds of at least "
            f"{args.calls} back-to-back products and {args.window_ms:g} ms each, device events, the routes alternating; spread = (max - min) / median over the rounds\n\n"
            + "\n".join(lines) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
