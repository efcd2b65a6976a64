"""Time the splat at query points: plx_query_plan, plx_splat_at / plx_splat_at_f64 (csrc/plx_query_adjoint.hip over the
kernels of csrc/plx_rows.hip / plx_rows_f64.hip) and query_adjoint.apply_at_t, at 1 / 101 columns, for n* = 1, 1e4, 1e5
held-out points, in fp32 and double, next to Lattice.splat_rows of the same row count and width: it runs the same kernels,
with its table made by a compaction of the build's sorted corners instead of a sort.

Method (that of tools/query_grad_time.py): device events around `calls` back-to-back calls, the MEDIAN over `rounds` rounds,
the calls alternating round by round in one process, after a warm-up of all of them; next to the median the spread (max - min
over the rounds, as a share of the median): a difference inside it says nothing.  splat_rows is timed on a warm range (its
table built by the warm-up); plan allocates its buffer in every call, as a backward does.

    python tools/query_adjoint_time.py [--out FILE.md] [--rounds 5] [--calls 20] [--points 1000000]

Shape: N = 1e6, d = 8, order 1.  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import query_adjoint  # noqa: E402

NSTAR = (1, 10_000, 100_000)
COLUMNS = (1, 101)


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


def measure(rounds, calls, n=1_000_000, d=8):
    dev = torch.device("cuda", 0)
    taps = plx.DiscretizedKernelFN(plx.rbf, 1).get_coeffs().numpy()
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=gen).to(dev)
    lat = plx.Lattice(dev).build(x, taps)
    lines = [f"N = {n}, d = {d}, order 1, m = {lat.m}", "",
             "| dtype | columns | n* | found share | plan ms (spread) | splat_at ms (spread) | splat_rows ms (spread) | "
             "apply_at_t ms (spread) | splat_at kernel |", "|---|---|---|---|---|---|---|---|---|"]
    for dtype in (torch.float32, torch.float64):
        for c in COLUMNS:
            for ns in NSTAR:
                xs = torch.randn(ns, d, generator=gen).to(dev)
                q = lat.locate(xs)
                share = float((q.vid >= 0).float().mean())
                g = torch.randn(ns, c, generator=gen).to(dev, dtype)
                plan = query_adjoint.plan(lat, q)
                values = lat.new_values(c, dtype)
                rows_values = lat.new_values(c, dtype)
                out = torch.empty(n, c, dtype=dtype, device=dev)
                runs = {"plan": lambda: query_adjoint.plan(lat, q),
                        "splat_at": lambda: query_adjoint.splat_at(lat, g, q, plan=plan, values=values),
                        "splat_rows": lambda: lat.splat_rows(g, 0, values=rows_values),
                        "apply_at_t": lambda: query_adjoint.apply_at_t(lat, g, q, plan=plan, out=out)}
                for fn in runs.values():
                    fn()
                    fn()
                torch.cuda.synchronize()
                times = {k: [] for k in runs}
                for _ in range(rounds):
                    for k, fn in runs.items():                        # alternating: every round times every call once
                        times[k].append(timed(fn, calls))
                query_adjoint.splat_at(lat, g, q, plan=plan, values=values)
                lines.append(f"| {str(dtype).split('.')[1]} | {c} | {ns} | {share:.3f} | " +
                             " | ".join(cell(times[k]) for k in runs) + f" | {query_adjoint.kernels(lat)['splat_at'][0]} |")
                del values, rows_values, out, plan
    lat.close()
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_adjoint_time.py needs a GPU: a CPU run says nothing about these kernels")
    text = (f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of {args.calls} back-to-back calls, "
            "device events, the calls alternating; spread = (max - min) / median over the rounds; held-out queries: a fresh "
            "draw of the cloud\n\n" + "\n".join(measure(args.rounds, args.calls, n=args.points)) + "\n")
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
