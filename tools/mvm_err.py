#!/usr/bin/env python3
"""The lattice against the exact kernel MVM on one MI355X: approximation error and time (the reference's
experiments/mvm_err.py, with plx_exact_mvm in place of KeOps).

For every bench.PUBLISHED_SHAPES entry and every BASELINE.json config shape (seeded randn stand-ins: x ~ N(0, I),
v ~ N(0, 1), t = 1), profiles rbf / Matern-3/2 / Matern-5/2, lengthscales 1 and 0.6931, lattice order 1..3:
  - rel_err / cos_err / rel_l2 of the lattice MVM against the exact one (exact.mvm_error);
  - warm ms per MVM of both paths (the lattice built once and reported apart);
  - the exact kernel's pairs/s against the VALU model of DESIGN.md section 9.
The exact output does not depend on the order: one exact MVM per (shape, profile, lengthscale).  A/B rules: a warm-up
call of each path first, then rounds in which the exact MVM and the three lattices alternate; the minimum over rounds
is reported (where one exact MVM is >= 1e12 pairs, that first call alone, after the smaller shapes).  A rate section times the exact kernel alone at
N = 1e5, d = 8, t = 1 and 11.

    python tools/mvm_err.py [--out profiles/mvm_err.md] [--shapes name,name] [--rounds 3] [--gpytorch-rbf] [--skip-rate]

--gpytorch-rbf divides the exact side's positions by sqrt(2) for the RBF profile: exp(-d2 / 2), GPyTorch's RBF, the
pairing the reference's published numbers come from (its lattice is exp(-d2)).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import simplex_gp_amd as plx  # noqa: E402
from bench import PUBLISHED_SHAPES  # noqa: E402

# BASELINE.json configs: Snelson 1-D (n = 200), config 1 (1e5, d = 4), configs 3 and 4 (1e6 / 4e6, d = 8), config 5
# (elevators' d = 18, its 16,599 rows)
CONFIG_SHAPES = [("config1 snelson", 200, 1), ("config2", 100_000, 4), ("config3", 1_000_000, 8), ("config4", 4_000_000, 8),
                 ("config5 elevators", 16_599, 18)]
PROFILES = [("rbf", None), ("matern32", 1.5), ("matern52", 2.5)]
ELLS = [1.0, 0.6931]
ORDERS = [1, 2, 3]
VALU_LANE_OPS = 3.9e13          # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz x ... (MI355X_MICROARCH constants), scalar VALU


def model_pairs_per_s(d, t, profile):
    """VALU model: per pair 2d lane-ops for the distance, 2 for v_exp_f32 (8 issue cycles against 4), t FMAs for the
    contraction, one for the loop; Matern adds a v_sqrt_f32 (2) and its polynomial (2)."""
    ops = 2 * d + 2 + t + 1 + (4 if profile != "rbf" else 0)
    return VALU_LANE_OPS / ops


def lattice_taps(profile, nu, order):
    k = plx.RBFLattice(order=order) if nu is None else plx.MaternLattice(nu=nu, order=order)
    return k.dkernel_fn.get_coeffs()


def timed(fn, reps):
    """Device ms per call of fn over reps back-to-back calls (events around them)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def run_shape(name, n, d, rounds, gpytorch_rbf, dev):
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=g).to(dev)
    v = torch.randn(n, 1, generator=g).to(dev)
    rows = []
    for profile, nu in PROFILES:
        for ell in ELLS:
            pos = (x / ell).contiguous()
            epos = (pos / math.sqrt(2)).contiguous() if (gpytorch_rbf and profile == "rbf") else pos
            pairs = float(n) * n
            single = pairs >= 1e12                      # one exact MVM is ~a second or more: time the first one only
            rr = 1 if single else rounds
            reps = 1 if pairs > 1e11 else (3 if pairs > 1e9 else 10)
            lats = {}
            for o in ORDERS:
                lat = plx.Lattice(dev)
                taps = lattice_taps(profile, nu, o)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lat.build(pos, taps)
                lat.prepare(1)
                torch.cuda.synchronize()
                build_ms = (time.perf_counter() - t0) * 1e3
                out = torch.empty_like(v)
                lat.apply(v, out)                                           # warm-up
                lats[o] = dict(lat=lat, out=out, build_ms=build_ms, ms=[])
            holder = {}
            first = timed(lambda: holder.setdefault("out", plx.exact_matmul(epos, epos, v, profile)), 1)
            exact = holder["out"]
            ems = [first] if single else []                                # the code is loaded: smaller shapes ran first
            for _ in range(rr):
                if not single:
                    ems.append(timed(lambda: plx.exact_matmul(epos, epos, v, profile), reps))
                for o in ORDERS:
                    L = lats[o]
                    L["ms"].append(timed(lambda: L["lat"].apply(v, L["out"]), 10 if n <= 2_000_000 else 3))
            ems = min(ems)
            for o in ORDERS:
                L = lats[o]
                e = plx.mvm_error(L["out"], exact)
                rows.append(dict(shape=name, n=n, d=d, profile=profile, ell=ell, order=o, m=L["lat"].m,
                                 rel_err=e["rel_err"], cos_err=e["cos_err"], rel_l2=e["rel_l2"],
                                 lattice_ms=min(L["ms"]), build_ms=L["build_ms"], exact_ms=ems,
                                 exact_pairs_per_s=pairs / (ems * 1e-3), model_pairs_per_s=model_pairs_per_s(d, 1, profile)))
                L["lat"].close()
            print(json.dumps(rows[-1]), flush=True)
    return rows


def rate_section(dev, rounds):
    """pairs/s of the exact kernel alone at N = 1e5, d = 8 (the DESIGN.md figures)."""
    out = []
    n, d = 100_000, 8
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=g).to(dev)
    for profile in ("rbf", "matern32"):
        for t in (1, 11):
            v = torch.randn(n, t, generator=g).to(dev)
            plx.exact_matmul(x, x, v, profile)
            ms = min(timed(lambda: plx.exact_matmul(x, x, v, profile), 5) for _ in range(rounds))
            rate = n * float(n) / (ms * 1e-3)
            out.append(dict(n=n, d=d, t=t, profile=profile, ms=ms, pairs_per_s=rate, model=model_pairs_per_s(d, t, profile)))
            print(json.dumps(out[-1]), flush=True)
    return out


def write_md(path, rows, rate, args, dev):
    lines = ["# Lattice vs exact kernel MVM on one MI355X", "",
             f"`tools/mvm_err.py{' --gpytorch-rbf' if args.gpytorch_rbf else ''}` on {torch.cuda.get_device_name(dev)}. "
             "Seeded stand-ins (x ~ N(0, I), v ~ N(0, 1), t = 1, seed 1234) at the shapes of the reference's published "
             "table and of BASELINE.json's configs; no UCI data. The exact side is `plx_exact_mvm` with the same profile "
             "as the lattice (exp(-d2) for rbf" + (", divided by sqrt 2 on the exact side: GPyTorch's exp(-d2/2)" if args.gpytorch_rbf
                                                    else "") + "). "
             "`rel_err` / `cos_err` are the reference's formulas (mean-ratio rescale first; cos_err is the cosine, 1 = "
             "same direction), `rel_l2` is the plain relative L2 error. Times: warm device ms per MVM, minimum over "
             "interleaved rounds (for exact MVMs of >= 1e12 pairs the single first call, the kernel code already loaded); `build` is the lattice build alone "
             "(host clock around a synchronised build + prepare). `model` is the VALU model of DESIGN.md section 9.", ""]
    if rate:
        lines += ["## Exact kernel rate, N = 1e5, d = 8", "", "| profile | t | ms | pairs/s | model pairs/s | of model |",
                  "|---|---|---|---|---|---|"]
        for r in rate:
            lines.append(f"| {r['profile']} | {r['t']} | {r['ms']:.3f} | {r['pairs_per_s']:.3e} | {r['model']:.2e} | "
                         f"{r['pairs_per_s'] / r['model']:.2f} |")
        lines.append("")
    lines += ["## Error and time per shape", "",
              "| shape | n | d | profile | ell | order | m | rel_err | cos_err | rel_l2 | lattice ms | build ms | exact ms | "
              "exact pairs/s | of model | exact / lattice |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {r['n']} | {r['d']} | {r['profile']} | {r['ell']} | {r['order']} | {r['m']} | "
                     f"{r['rel_err']:.4f} | {r['cos_err']:.4f} | {r['rel_l2']:.4f} | {r['lattice_ms']:.3f} | "
                     f"{r['build_ms']:.2f} | {r['exact_ms']:.2f} | {r['exact_pairs_per_s']:.3e} | "
                     f"{r['exact_pairs_per_s'] / r['model_pairs_per_s']:.2f} | {r['exact_ms'] / r['lattice_ms']:.0f}x |")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvm_err.md"))
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gpytorch-rbf", action="store_true")
    ap.add_argument("--skip-rate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mvm_err.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    shapes = [(name, n, d) for name, n, d, _ in PUBLISHED_SHAPES] + CONFIG_SHAPES
    if args.shapes:
        want = set(args.shapes.split(","))
        shapes = [s for s in shapes if s[0] in want or s[0].split()[0] in want]
    rate = [] if args.skip_rate else rate_section(dev, args.rounds)
    rows = []
    for name, n, d in sorted(shapes, key=lambda s: s[1]):
        rows += run_shape(name, n, d, args.rounds, args.gpytorch_rbf, dev)
    write_md(args.out, rows, rate, args, dev)


if __name__ == "__main__":
    main()
