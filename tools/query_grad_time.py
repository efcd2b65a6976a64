"""Time the position gradient of a query: plx_slice_at_dots (csrc/plx_query_kernels.h) and plx_locate_pullback
(locate_pullback_kernel, csrc/plx_build.hip) at 1 / 101 columns, for n* = 1, 1e4, 1e5 held-out points, in fp32 and double,
next to the forward they differentiate (plx_locate, plx_slice_at); then one differentiable prediction --
PredictionCache.predict_query_grad and the backward of mean.sum() + var.sum() -- against the only other way to the same
derivative: the stacked route's formulas run with a graph (RectangularLazyLattice over [x*; X], a lattice built per batch)
and their backward (the filter position gradient).  The stacked code is not touched by the query gradient, hence the yardstick.

Method (that of tools/query_time.py): device events around `calls` back-to-back calls, the MEDIAN over `rounds` rounds, the
calls alternating round by round in one process, after a warm-up of all of them; next to the median the spread (max - min
over the rounds, as a share of the median): a difference inside it says nothing.  A prediction is timed one call per round.

    python tools/query_grad_time.py [--out FILE.md] [--rounds 5] [--calls 20] [--lanczos 100] [--no-kernels] [--no-predict]

Shape: N = 1e6, d = 8, order 1.  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import _native as nv  # noqa: E402
from simplex_gp_amd import query_grad, solvers, training  # noqa: E402

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


def measure_kernels(rounds, calls, n=1_000_000, d=8):
    dev = torch.device("cuda", 0)
    taps = plx.DiscretizedKernelFN(plx.rbf, 1).get_coeffs().numpy()
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=gen).to(dev)
    lat = plx.Lattice(dev).build(x, taps)
    lines = [f"N = {n}, d = {d}, order 1, m = {lat.m}", "",
             "| dtype | columns | n* | found share | locate ms (spread) | slice_at ms (spread) | slice_at_dots ms (spread) | "
             "locate_pullback ms (spread) | dots kernel |", "|---|---|---|---|---|---|---|---|---|"]
    for dtype in (torch.float32, torch.float64):
        for c in COLUMNS:
            values, _ = lat.blurred(torch.randn(n, c, generator=gen).to(dev, dtype))
            for ns in NSTAR:
                xs = torch.randn(ns, d, generator=gen).to(dev)
                q = lat.locate(xs)
                share = float((q.vid >= 0).float().mean())
                g = torch.randn(ns, c, generator=gen).to(dev, dtype)
                t = query_grad.slice_at_dots(lat, values, q, g, vd=c)
                out = torch.empty(ns, c, dtype=dtype, device=dev)
                runs = {"locate": lambda: lat.locate(xs),
                        "slice_at": lambda: lat.slice_at(values, q, out=out, vd=c),
                        "dots": lambda: query_grad.slice_at_dots(lat, values, q, g, vd=c),
                        "pullback": lambda: query_grad.locate_pullback(lat, q, t)}
                for fn in runs.values():
                    fn()
                    fn()
                torch.cuda.synchronize()
                times = {k: [] for k in runs}
                for _ in range(rounds):
                    for k, fn in runs.items():                        # alternating: every round times every call once
                        times[k].append(timed(fn, calls))
                lines.append(f"| {str(dtype).split('.')[1]} | {c} | {ns} | {share:.3f} | " +
                             " | ".join(cell(times[k]) for k in runs) + f" | {query_grad.kernels(lat)['dots'][0]} |")
            del values
    lat.close()
    torch.cuda.empty_cache()
    return lines


def measure_predict(rounds, n=1_000_000, d=8, lanc=100):
    """One PredictionCache (rank-100 preconditioner, `lanc` Lanczos steps) on the shape; forward + backward of
    mean.sum() + var.sum() with respect to x*, by the query route and by the stacked formulas with a graph."""
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(n, d, generator=gen).to(dev)
    y = (torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=gen).to(dev))
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).to(dev)
    cache = training.PredictionCache(model, x, y, lanc_iter=lanc, pre_size=100)
    model.requires_grad_(False)                       # x* alone is differentiated, by either route
    AQ = torch.cat([cache.alpha, cache.Q], 1).contiguous()

    def query(xs):
        xg = xs.clone().requires_grad_(True)
        mean, var = cache.predict_query_grad(xg)
        (mean.sum() + var.sum()).backward()
        return xg.grad

    def stacked(xs):
        xg = xs.clone().requires_grad_(True)
        s = model.outputscale.detach()
        KAQ = s * model.kernel(xg, cache.x).matmul(AQ)
        mean = model.mean.detach() + KAQ[:, 0]
        proj = torch.linalg.solve_triangular(cache.chol, KAQ[:, 1:].t(), upper=False)
        var = (s - (proj ** 2).sum(0)).clamp_min(1e-8)
        (mean.sum() + var.sum()).backward()
        return xg.grad

    lines = [f"N = {n}, d = {d}, RBF order 1, 1 + {cache.Q.shape[1]} columns", "",
             "| n* | stacked forward + backward ms (spread) | predict_query_grad + backward ms (spread) | stacked / query | "
             "no-graph predict(route=\"query\") ms (spread) |", "|---|---|---|---|---|"]
    for ns in NSTAR:
        xs = torch.randn(ns, d, generator=gen).to(dev)
        runs = {"stacked": lambda: stacked(xs), "query": lambda: query(xs), "plain": lambda: cache.predict(xs, route="query")}
        refused = None
        try:
            stacked(xs)
        except nv.PlxError as e:                          # the stack of the filter gradient has 2 (1 + d) columns per column
            refused = str(e)
            del runs["stacked"]
        for fn in runs.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                times[k].append(timed(fn, 1))
        if refused is None:
            ratio = f"{statistics.median(times['stacked']) / statistics.median(times['query']):.1f}"
            lines.append(f"| {ns} | {cell(times['stacked'])} | {cell(times['query'])} | {ratio} | {cell(times['plain'])} |")
        else:
            lines.append(f"| {ns} | refused: {refused} | {cell(times['query'])} | - | {cell(times['plain'])} |")
    del cache, model, x, y
    plx.lattice_cache().clear()
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--lanczos", type=int, default=100)
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_grad_time.py needs a GPU: a CPU run says nothing about these kernels")

    def emit(text, mode):
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, mode) as f:
                f.write(text)

    emit(f"device: {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds of {args.calls} back-to-back calls, "
         "device events, the calls alternating; spread = (max - min) / median over the rounds; held-out queries: a fresh "
         "draw of the cloud\n", "w")
    if not args.no_kernels:
        emit("\n" + "\n".join(measure_kernels(args.rounds, args.calls, n=args.points)) + "\n", "a")
    if not args.no_predict:
        emit("\nOne differentiable prediction (forward and backward of mean.sum() + var.sum() in x*), one call per round, "
             "both on one cache\n\n" + "\n".join(measure_predict(args.rounds, n=args.points, lanc=args.lanczos)) + "\n", "a")


if __name__ == "__main__":
    main()
