"""How good is a slice of the training lattice at held-out points?  For each shape: the share of query corners the
training lattice holds and the distribution of the per-query weight mass (Lattice.locate), then, for one right-hand side
v, the three products at the held-out points x*

    query    K_q(x*, X) v = S* B S_X^T v / (1 + 2^-d)     Lattice.apply_at on the lattice of X
    stacked  K(x*, X) v on the lattice of [x*; X]          Lattice.apply_rows: what RectangularLazyLattice computes
    exact    sum_j k(|x*_i - x_j|^2) v_j                    exact.exact_matmul, the kernel both approximate

compared pairwise with exact.mvm_error (rel-L2 without rescaling, the reference's rescaled rel_err, the cosine).  v is the
"mean" column: positive and smooth (1 + 0.5 sin(sum x)), so that the products do not cancel and a relative error means
something.  The same at three lengthscales, because the found share is a property of how coarse the lattice is.

    python tools/query_err.py [--out profiles/query_err.md] [--nstar 10000]

Shapes: N = 1e6, d = 8, order 1 (RBF); the config-5 stand-in (Matern-3/2, order 3, N = 10,623, d = 18).  Needs a GPU.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import exact  # noqa: E402


def shapes():
    rbf1 = plx.DiscretizedKernelFN(plx.rbf, 1).get_coeffs().numpy()
    taps5 = plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18).dkernel_fn.get_coeffs().numpy()
    return [("N = 1e6, d = 8, RBF order 1", 1_000_000, 8, rbf1, "rbf"),
            ("N = 10,623, d = 18, Matern-3/2 order 3 (config-5 stand-in)", 10_623, 18, taps5, "matern32")]


def measure(nstar):
    dev = torch.device("cuda", 0)
    q = torch.tensor([0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0], device=dev)
    lines = ["| shape | lengthscale | m / (N (d+1)) | found share | mass: min / 5 % / 25 % / median / 75 % / 95 % / max | "
             "share of queries with mass 0 | query vs stacked: rel-L2 | query vs exact: rel-L2 / rel_err / cos | "
             "stacked vs exact: rel-L2 / rel_err / cos |", "|---|---|---|---|---|---|---|---|---|"]
    for name, n, d, taps, profile in shapes():
        gen = torch.Generator().manual_seed(4321)
        x0 = torch.randn(n, d, generator=gen).to(dev)
        xs0 = torch.randn(nstar, d, generator=gen).to(dev)
        for ell in (2.0, 1.0, 0.5):
            x, xs = (x0 / ell).contiguous(), (xs0 / ell).contiguous()
            v = (1.0 + 0.5 * torch.sin(x0.sum(1, keepdim=True))).contiguous()
            lat = plx.Lattice(dev).build(x, taps)
            loc = lat.locate(xs)
            share = float((loc.vid >= 0).float().mean())
            mass = torch.quantile(loc.mass, q).tolist()
            zero = float((loc.mass == 0).float().mean())
            by_query = lat.apply_at(v, loc)
            fill = lat.m / (n * (d + 1))
            lat.close()
            stacked_lat = plx.Lattice(dev).build(torch.cat([xs, x], 0).contiguous(), taps)
            by_stack = stacked_lat.apply_rows(v, nstar, 0, nstar)
            stacked_lat.close()
            want = exact.exact_matmul(xs, x, v, profile)
            qe, se = exact.mvm_error(by_query, want), exact.mvm_error(by_stack, want)
            qs = float((by_query - by_stack).double().norm() / by_stack.double().norm())
            lines.append(f"| {name} | {ell} | {fill:.3f} | {share:.3f} | " + " / ".join(f"{m:.3f}" for m in mass) +
                         f" | {zero:.3f} | {qs:.3e} | {qe['rel_l2']:.3e} / {qe['rel_err']:.3e} / {qe['cos_err']:.5f} | "
                         f"{se['rel_l2']:.3e} / {se['rel_err']:.3e} / {se['cos_err']:.5f} |")
            del lat, stacked_lat, by_query, by_stack, want
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--nstar", type=int, default=10_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_err.py needs a GPU")
    text = (f"device: {torch.cuda.get_device_name(0)}; {args.nstar} held-out queries (a fresh draw of the Gaussian cloud), "
            "positions divided by the lengthscale, one positive right-hand side\n\n" + "\n".join(measure(args.nstar)) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
