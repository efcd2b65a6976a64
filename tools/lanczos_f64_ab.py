"""A/B of the float64 Lanczos step (plx_lanczos_step_f64) against the two torch forms a double v0 took before it, on the
double model's own operator (LatticeGP.khat_in_lattice_rows), in ONE process with the forms interleaved:

    native    training.lanczos(mm, v0, steps)                            (LANCZOS_NATIVE_F64 = True)
    eager     training.lanczos(mm, v0, steps, graph=False, native=False) the torch loop
    replayed  training.lanczos(mm, v0, steps) with LANCZOS_NATIVE_F64 = False, where lanczos picks the captured graph
              (steps >= LANCZOS_GRAPH_MIN_STEPS, n <= LANCZOS_GRAPH_MAX_ROWS)

at the config-5 stand-in (N = 10,623, d = 18, Matern-3/2 order 3) and at N = 1e6, d = 8 (RBF order 1); then one
PredictionCache build + predict of the double model with the switch on and off.  Medians of `rounds` runs after one
warm-up round; a host clock around work that ends in a device synchronise.  One JSON line per measurement.

    timeout -k 10 900 python tools/lanczos_f64_ab.py [--rounds 5] [--steps 100] [--small-only]

No retries: a failure ends the run."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx                                              # noqa: E402
from simplex_gp_amd import solvers, training                              # noqa: E402


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def with_switch(on, f):
    was = training.LANCZOS_NATIVE_F64
    training.LANCZOS_NATIVE_F64 = on
    try:
        return f()
    finally:
        training.LANCZOS_NATIVE_F64 = was


def medians(forms, rounds):
    """{label: (median ms, min, max)} of `rounds` interleaved runs after one warm-up round."""
    times = {k: [] for k in forms}
    for r in range(rounds + 1):
        for label, f in forms.items():
            t, _ = timed(f)
            if r:
                times[label].append(t)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--small-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lanczos_f64_ab.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    shapes = [("config-5 stand-in", 10_623, 18, lambda d: plx.MaternLattice(nu=1.5, order=3, ard_num_dims=d)),
              ("N = 1e6", 1_000_000, 8, lambda d: plx.RBFLattice(order=1, ard_num_dims=d))]
    for name, n, d, kern in shapes[:1 if args.small_only else 2]:
        g = torch.Generator().manual_seed(1234)
        x = torch.randn(n, d, generator=g, dtype=torch.float64).to(dev)
        r = torch.randn(n, 1, generator=g, dtype=torch.float64).to(dev)
        model = solvers.LatticeGP(kern(d), min_noise=0.1).double().to(dev)
        steps = args.steps
        with torch.no_grad(), model.khat_in_lattice_rows(x) as (mm, to_rows, from_rows):
            v0 = to_rows(r).squeeze(-1)
            forms = {"native": lambda: with_switch(True, lambda: training.lanczos(mm, v0, steps)),
                     "eager": lambda: training.lanczos(mm, v0, steps, graph=False, native=False)}
            if steps >= training.LANCZOS_GRAPH_MIN_STEPS and n <= training.LANCZOS_GRAPH_MAX_ROWS:
                forms["replayed"] = lambda: with_switch(False, lambda: training.lanczos(mm, v0, steps))
            forms["mvm only"] = lambda: [mm(v0.unsqueeze(-1)) for _ in range(steps)]
            res = medians(forms, args.rounds)
            # the same recurrence: T of the native form against the eager one
            Tn = with_switch(True, lambda: training.lanczos(mm, v0, steps))[1]
            Te = training.lanczos(mm, v0, steps, graph=False, native=False)[1]
            k = min(10, Tn.shape[0], Te.shape[0])
            gap = float((Tn[:k, :k] - Te[:k, :k]).abs().max() / Te[0, 0].abs())
        print(json.dumps({"what": f"{steps} Lanczos steps, float64", "shape": name, "n": n, "d": d, "rounds": args.rounds,
                          "median_ms [min, max]": {k: [round(v, 3) for v in t] for k, t in res.items()},
                          "refusals": list(training._graph_refusals), "leading_T_gap_native_vs_eager": gap}), flush=True)
        # one PredictionCache build + predict, switch on and off
        xs = torch.randn(min(n // 4, 10_000), d, generator=g, dtype=torch.float64).to(dev)
        y = torch.sin(x.sum(1)) + 0.1 * r.squeeze(-1)

        def cache_and_predict():
            return training.PredictionCache(model, x, y, lanc_iter=steps).predict(xs)

        res = medians({"switch on": lambda: with_switch(True, cache_and_predict),
                       "switch off": lambda: with_switch(False, cache_and_predict)}, max(3, args.rounds // 2))
        print(json.dumps({"what": "PredictionCache(...) + predict, double model", "shape": name, "n": n, "d": d,
                          "test_rows": int(xs.shape[0]),
                          "median_ms [min, max]": {k: [round(v, 3) for v in t] for k, t in res.items()}}), flush=True)
        del model, x, r, xs, y
        plx.lattice_cache().clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
