"""Time the float64 exact kernel MVM (plx_exact_mvm_f64) next to the fp32 one (plx_exact_mvm), and record the two errors the
double kernel makes measurable: the fp32 exact kernel's own error, and the float64 lattice product's distance from the exact
product.

Method (that of tools/cg_f64_time.py): device events around `calls` back-to-back MVMs, the minimum over `rounds` rounds, the
fp32 and the float64 kernel alternating round by round in one process on the same points, after a warm-up of both.  Next to
the minimum the spread (max - min over the rounds, as a share of the minimum) is recorded: a difference inside it says
nothing.  There is no pass / fail threshold on any time.

Shape: DESIGN.md section 9's, N = 1e5, d = 8, square; rbf and matern32; t = 1 and 11.  Per row: ms per MVM and pairs/s of
both kernels, float64 / fp32, and the double kernel's share of its cost model (model_pairs_per_s_f64: the VALU instructions
of the inner loop as counted in the ISA, a double-rate instruction priced at two fp32 issue slots -- the datasheet's ratio
of the FP64 to the FP32 vector peak, an assumption this table tests, not a measured rate).
rel_l2 fp32 vs float64: |out32 - out64| / |out64| of the two exact kernels on the SAME fp32-representable inputs: the fp32
yardstick's own error.
Lattice vs exact, float64: mvm_error of the float64 lattice product (RBFLattice order 1 on a double model) against the
float64 exact product at N = 20,000, d = 4.

    python tools/exact_f64_time.py [--out profiles/exact_f64_measured.md] [--rounds 5] [--calls 3] [--n 100000]

Needs a GPU: there is no CPU timing.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402

VALU_LANE_OPS = 3.93e13          # fp32 lane-ops/s: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
DPS, TCS = (4, 8, 12, 16, 20, 24, 32), (1, 4, 8, 16)


def model_pairs_per_s_f64(d, t, profile):
    """The inner loop of exact_mvm_kernel<double, ...> as compiled: per pair and lane 2 DP double-rate
    instructions for the distance, 20 for the software exp (v_mul, v_rndne, 14 FMAs of the reduction and the polynomial,
    v_cvt_i32_f64, v_ldexp_f64, two compares), TC FMAs for the contraction, and 13 single-rate ones (the polynomial's
    constants as v_mov_b64, the range selects, the loop); a Matern adds 17 double-rate (v_rsq_f64 and its Newton steps,
    two v_ldexp_f64, the scaling and the polynomial) and 5 single-rate.  A double-rate instruction takes two issue slots."""
    dp = next((x for x in DPS if d <= x), DPS[-1])
    tc = next((x for x in TCS if t <= x), TCS[-1])
    matern = profile != "rbf"
    double = 2 * dp + 20 + tc + (17 if matern else 0)
    single = 13 + (5 if matern else 0)
    blocks = -(-t // tc)                                     # the forward recomputes k per column block
    return VALU_LANE_OPS / ((2 * double + single) * blocks)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--n", type=int, default=100_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exact_f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda", 0)
    n, d = args.n, 8
    g = torch.Generator().manual_seed(1234)
    x32 = (torch.randn(n, d, generator=g) * (2.0 / math.sqrt(d))).to(dev)
    x64 = x32.double()                                       # the same, fp32-representable, values for both kernels
    lines = ["| profile | t | fp32 ms (spread) | fp32 pairs/s | float64 ms (spread) | float64 pairs/s | float64 / fp32 | model pairs/s "
             "| of model | rel_l2 fp32 vs float64 |", "|---|---|---|---|---|---|---|---|---|---|"]
    for profile in ("rbf", "matern32"):
        for t in (1, 11):
            v32 = torch.randn(n, t, generator=g).to(dev)
            v64 = v32.double()
            runs = {"fp32": lambda: plx.exact_matmul(x32, x32, v32, profile),
                    "float64": lambda: plx.exact_matmul(x64, x64, v64, profile)}
            with torch.no_grad():
                outs = {k: fn() for k, fn in runs.items()}   # warm-up of both: code objects, the allocator's blocks
                for fn in runs.values():
                    fn()
                torch.cuda.synchronize()
                times = {k: [] for k in runs}
                for _ in range(args.rounds):
                    for k, fn in runs.items():               # alternating: every round times both once
                        times[k].append(timed(fn, args.calls))
            assert outs["fp32"].dtype == torch.float32 and outs["float64"].dtype == torch.float64
            assert bool(torch.isfinite(outs["float64"]).all())
            best = {k: min(v) for k, v in times.items()}
            cell = lambda k: f"{best[k]:.2f} ({(max(times[k]) - best[k]) / best[k] * 100:.1f} %)"      # noqa: E731
            rate = {k: n * n / (best[k] * 1e-3) for k in best}
            model = model_pairs_per_s_f64(d, t, profile)
            lines.append(f"| {profile} | {t} | {cell('fp32')} | {rate['fp32']:.3g} | {cell('float64')} | {rate['float64']:.3g} | "
                         f"{best['float64'] / best['fp32']:.2f} | {model:.3g} | {rate['float64'] / model:.2f} | "
                         f"{rel_l2(outs['fp32'], outs['float64']):.2e} |")
            print(lines[-1], flush=True)
    # the float64 lattice product against the float64 exact one
    nl, dl = 20_000, 4
    xl = (torch.randn(nl, dl, generator=g, dtype=torch.float64) * 1.5).to(dev)
    w = torch.randn(dl, 1, generator=g, dtype=torch.float64).to(dev)
    vl = torch.sin(xl @ w) + 0.5                             # smooth in the positions
    lat = plx.RBFLattice(order=1).double().to(dev)
    lat.lengthscale = 1.0
    twin = plx.exact_twin(lat)
    with torch.no_grad():
        a, b = lat(xl, xl) @ vl, twin(xl, xl) @ vl
    assert a.dtype == torch.float64 and b.dtype == torch.float64
    e = plx.mvm_error(a, b)
    text = (f"device: {torch.cuda.get_device_name(0)}; exact K(x, x) v, N = {n}, d = {d}; minimum of {args.rounds} rounds of "
            f"{args.calls} MVMs, device events, the fp32 and the float64 kernel alternating; spread = (max - min) / min over the "
            "rounds; model: tools/exact_f64_time.py model_pairs_per_s_f64 (a double-rate instruction priced at two fp32 issue "
            "slots: an assumption, not a measured rate)\n\n" + "\n".join(lines) + "\n\n"
            f"float64 lattice product (RBFLattice, order 1, lengthscale 1) against the float64 exact product, N = {nl}, d = {dl}, "
            f"t = 1: rel_err {e['rel_err']:.4e}, cos_err {e['cos_err']:.6f}, rel_l2 {e['rel_l2']:.4e}\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
