"""Time the symmetrised float64 product: plx_apply_sym_f64 (one splat, d + 1 launches that advance both blur chains, one
slice) next to plx_apply_f64 + plx_apply_t_f64 back to back (the two full products it replaces) and next to one
plx_apply_f64 (what a solve on K itself pays per iteration).

Method (that of tools/backward_f64_time.py): device events around `calls` back-to-back products, the minimum over `rounds`
rounds, the routes alternating round by round in one process on one lattice, after a warm-up of all of them.  Next to the
minimum the spread (max - min over the rounds, as a share of the minimum) is recorded: a difference inside it says nothing.

    python tools/sym_f64_time.py [--out profiles/sym_f64_time.md] [--rounds 7] [--calls 20] [--parent-library PATH]

--parent-library: a libplx.so built from the parent commit.  One plx_apply_f64 is then timed on it as well, in a child
process of its own (PLX_LIBRARY selects the library when simplex_gp_amd._native is first imported), on the same shapes with
the same seeds.

Shapes: those of tools/backward_f64_time.py with the kernels' own (forward) taps: N = 1e6, d = 8, order 1; N = 2e4, d = 4,
order 1; the config-5 stand-in (MaternLattice nu = 1.5, order 3, N = 10,623, d = 18); widths 1 and 12.  Needs a GPU.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402

WIDTHS = (1, 12)


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


def measure(plain_only, rounds, calls):
    """{(shape name, vd): {route: [ms per round]}} and the vertex counts."""
    dev = torch.device("cuda", 0)
    out, ms = {}, {}
    for name, n, d, taps in shapes():
        gen = torch.Generator().manual_seed(1234)
        x = torch.randn(n, d, generator=gen).to(dev)
        lat = plx.Lattice(dev).build(x, taps)
        ms[name] = lat.m
        for vd in WIDTHS:
            v = torch.randn(n, vd, generator=gen, dtype=torch.float64).to(dev)
            o1, o2 = torch.empty_like(v), torch.empty_like(v)
            runs = {"plain": lambda: lat.apply(v, out=o1)}
            if not plain_only:
                runs["sym"] = lambda: lat.apply_sym(v, out=o1)
                runs["pair"] = lambda: (lat.apply(v, out=o1), lat.apply_t(v, out=o2))
            for fn in runs.values():                                  # warm-up: workspaces grown, tables built
                fn()
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(rounds):
                for k, fn in runs.items():                            # alternating: every round times every route once
                    times[k].append(timed(fn, calls))
            out[f"{name} | {vd}"] = times
            del v, o1, o2
        lat.close()
        del x
        torch.cuda.empty_cache()
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--plain-only-json", action="store_true", help="(internal) time plx_apply_f64 alone, print JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sym_f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    if args.plain_only_json:
        times, _ = measure(True, args.rounds, args.calls)
        print("PLAIN_JSON " + json.dumps(times))
        return
    times, ms = measure(False, args.rounds, args.calls)
    parent = None
    if args.parent_library:
        env = dict(os.environ, PLX_LIBRARY=os.path.abspath(args.parent_library))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only-json", "--rounds", str(args.rounds),
                              "--calls", str(args.calls)], env=env, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit(f"the run on {args.parent_library} failed:\n{res.stdout}\n{res.stderr}")
        parent = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("PLAIN_JSON ")][-1][len("PLAIN_JSON "):])

    def cell(ts):
        best = min(ts)
        return f"{best:.4f} ({(max(ts) - best) / best * 100:.1f} %)"

    lines = ["| shape | m | columns | apply_sym ms (spread) | apply + apply_t ms (spread) | one apply ms (spread) | "
             "one apply, parent library ms (spread) | sym / (apply + apply_t) | sym / one apply |",
             "|---|---|---|---|---|---|---|---|---|"]
    for key, t in times.items():
        name, vd = key.rsplit(" | ", 1)
        sym, pair, plain = min(t["sym"]), min(t["pair"]), min(t["plain"])
        pcell = cell(parent[key]["plain"]) if parent else "not run"
        lines.append(f"| {name} | {ms[name]} | {vd} | {cell(t['sym'])} | {cell(t['pair'])} | {cell(t['plain'])} | {pcell} | "
                     f"{sym / pair:.2f} | {sym / plain:.2f} |")
    text = (f"device: {torch.cuda.get_device_name(0)}; float64 right-hand sides; minimum of {args.rounds} rounds of {args.calls} "
            "back-to-back products, device events, the routes alternating; spread = (max - min) / min over the rounds\n\n"
            + "\n".join(lines) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
