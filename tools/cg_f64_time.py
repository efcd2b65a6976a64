"""Time one float64 CG iteration (MVM + update + direction) on the native double kernels next to the torch formulation.

Method (that of tools/f64_time.py): device events around `calls` back-to-back iterations, the minimum over `rounds` rounds,
the variants alternating round by round in one process on one lattice, after a warm-up of all of them.  Next to the minimum
the spread (max - min over the rounds, as a share of the minimum) is recorded: a difference inside it says nothing.

Variants, per shape, 12 columns of doubles:
    native            apply_affine(want_dot=True) + plx_cg_step_update_f64 + plx_cg_step_direction_f64
    torch             the loop body batched_cg runs with solvers.NATIVE_CG_F64 = False (what it ran before the native double
                      iteration existed): lat.apply(V).mul_(s).addcmul_(V, noise), (P * AP).sum(0), two addcmul_, (R * R).sum(0),
                      the coefficient and mask expressions, P.mul_(beta).add_(R)
    native vectors    the vector work alone: plx_coldot_f64(P, AP) + the two native steps (the MVM excluded; the stand-alone
                      dot is counted although the full iteration gets it from the slice kernel)
    torch vectors     the torch loop body without its MVM
The MVM in double is dominated by the fp64 splat on coarse lattices (3 ms at the headline shape), which
hides the vector work in the full-iteration columns; the two "vectors" columns are what this change is about.

    python tools/cg_f64_time.py [--out profiles/cg_f64_time.md] [--rounds 7] [--calls 20]
    python tools/cg_f64_time.py --fp32 [--rounds 7] [--calls 20]      the fp32 vector calls alone (plx_coldot + plx_cg_step_update
                                                                     + plx_cg_step_direction), n of the three shapes, vd = 11 and 12

Shapes: N = 1e6, d = 8, order 1 (the headline build); N = 2e4, d = 4, order 1; the config-5 stand-in (MaternLattice nu = 1.5,
order 3, N = 10,623, d = 18).  Needs a GPU: there is no CPU timing.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import _native as nv  # noqa: E402
from simplex_gp_amd import solvers  # noqa: E402

VD = 12


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


class Iteration:
    """The state of a batched CG run on (s K + noise I) X = B in double, and one iteration of it per variant.  alpha is
    scaled down so that a few hundred timed iterations move the vectors by rounding-level amounts only (the timing does
    not depend on the values; overflow would)."""

    def __init__(self, lat, n, seed):
        g = torch.Generator().manual_seed(seed)
        dev = lat.device
        self.lat, self.n = lat, n
        self.B = torch.randn(n, VD, generator=g, dtype=torch.float64).to(dev)
        self.s = torch.tensor(0.7, dtype=torch.float64, device=dev)
        self.noise = torch.tensor(1.0, dtype=torch.float64, device=dev)
        self.ss = torch.stack([self.s, self.noise]).contiguous()
        self.X, self.R, self.P = torch.zeros_like(self.B), self.B.clone(), self.B.clone()
        self.AP = lat.apply_affine(self.P, self.ss)
        self.rs = solvers._colsum(self.R, self.R).clone()
        self.rs_new = torch.empty_like(self.rs)
        self.b_norm = self.rs.sqrt()
        self.pap = solvers._colsum(self.P, self.AP).clone() * 1e12        # alpha ~ 1e-12
        self.active = torch.ones(VD, dtype=torch.float64, device=dev)
        self.active_next = torch.empty_like(self.active)
        self.alpha, self.beta = torch.empty_like(self.rs), torch.empty_like(self.rs)
        self.work = torch.empty(int(nv.lib().plx_coldot_work_doubles(VD)), dtype=torch.float64, device=dev)
        self.active_b = torch.ones(VD, dtype=torch.bool, device=dev)

    def native_vectors(self, with_dot=True):
        lib, n = nv.lib(), self.n
        p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if with_dot:
            nv.check(lib.plx_coldot_f64(p(self.P), p(self.AP), n, VD, p(self.rs_new), p(self.work), st), "plx_coldot_f64")
        nv.check(lib.plx_cg_step_update_f64(p(self.X), p(self.R), p(self.P), p(self.AP), p(self.rs), p(self.pap), p(self.active), n,
                                            VD, p(self.rs_new), p(self.alpha), p(self.work), st), "plx_cg_step_update_f64")
        nv.check(lib.plx_cg_step_direction_f64(p(self.P), p(self.R), p(self.rs_new), p(self.rs), p(self.active), p(self.b_norm),
                                               0.0, n, VD, p(self.beta), p(self.active_next), st), "plx_cg_step_direction_f64")

    def native(self):
        self.lat.apply_affine(self.P, self.ss, out=self.AP, want_dot=True)
        self.native_vectors(with_dot=False)

    def torch_vectors(self):
        X, R, P, AP, rs, active = self.X, self.R, self.P, self.AP, self.rs, self.active_b
        pAp = (P * AP).sum(0) * 1e12
        alpha = torch.where(active, rs / pAp.clamp_min(1e-30), torch.zeros_like(rs))
        X.addcmul_(P, alpha)
        R.addcmul_(AP, -alpha)
        rs_new = (R * R).sum(0)
        beta = torch.where(active, rs_new / rs.clamp_min(1e-30), torch.zeros_like(rs))
        P.mul_(beta).add_(R)
        self.active_b = active & (rs_new.sqrt() / self.b_norm > 0.0)

    def torch(self):
        self.AP = self.lat.apply(self.P).mul_(self.s).addcmul_(self.P, self.noise).contiguous()
        self.torch_vectors()


def fp32_vectors(rounds, calls):
    """The fp32 twins of "native vectors": plx_coldot + plx_cg_step_update + plx_cg_step_direction on [n][vd] floats, n of
    the three shapes, vd = 11 (the scalar direction kernel at odd n) and 12 (the vector one); no lattice is needed."""
    lib, dev = nv.lib(), torch.device("cuda", 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("| n | vd | fp32 vectors ms (spread) |\n|---|---|---|")
    for n in (1_000_000, 20_000, 10_623):
        for vd in (11, 12):
            g = torch.Generator().manual_seed(n + vd)
            X, R, P, AP = (torch.randn(n, vd, generator=g).to(dev) for _ in range(4))
            rs, b_norm, active = (R * R).sum(0), R.norm(dim=0), torch.ones(vd, device=dev)
            pap = (P * AP).sum(0).abs() * 1e12 + 1.0          # alpha ~ 1e-12: the vectors move by rounding-level amounts only
            rs_new, alpha, beta, active_next = (torch.empty(vd, device=dev) for _ in range(4))
            work = torch.empty(int(lib.plx_coldot_work_floats(vd)), device=dev)

            def step():
                nv.check(lib.plx_coldot(p(P), p(AP), n, vd, p(rs_new), p(work), st), "plx_coldot")
                nv.check(lib.plx_cg_step_update(p(X), p(R), p(P), p(AP), p(rs), p(pap), p(active), n, vd, p(rs_new), p(alpha), p(work),
                                                st), "plx_cg_step_update")
                nv.check(lib.plx_cg_step_direction(p(P), p(R), p(rs_new), p(rs), p(active), p(b_norm), 0.0, n, vd, p(beta),
                                                   p(active_next), st), "plx_cg_step_direction")
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            times = [timed(step, calls) for _ in range(rounds)]
            assert bool(torch.isfinite(X).all() and torch.isfinite(P).all())
            print(f"| {n} | {vd} | {min(times):.4f} ({(max(times) - min(times)) / min(times) * 100:.1f} %) |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--fp32", action="store_true", help="time the fp32 vector calls alone (no lattice, no torch route)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cg_f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    if args.fp32:
        return fp32_vectors(args.rounds, args.calls)
    dev = torch.device("cuda", 0)
    headline = np.array([0.34608543, 1.0, 0.34608543], np.float32)
    taps5 = plx.MaternLattice(nu=1.5, order=3, ard_num_dims=18).dkernel_fn.get_coeffs().numpy()
    shapes = [("N = 1e6, d = 8, order 1", 1_000_000, 8, headline), ("N = 2e4, d = 4, order 1", 20_000, 4, headline),
              ("N = 10,623, d = 18, order 3 (config-5 stand-in)", 10_623, 18, taps5)]
    names = ("native", "torch", "native vectors", "torch vectors")
    lines = ["| shape | m | " + " | ".join(f"{k} ms (spread)" for k in names) + " | torch / native | torch / native, vectors |",
             "|---|---|" + "---|" * (len(names) + 2)]
    for name, n, d, taps in shapes:
        x = torch.randn(n, d, generator=torch.Generator().manual_seed(1234)).to(dev)
        lat = plx.Lattice(dev).build(x, taps)
        it = Iteration(lat, n, seed=d)
        runs = {"native": it.native, "torch": it.torch, "native vectors": it.native_vectors, "torch vectors": it.torch_vectors}
        for fn in runs.values():                                  # warm-up: tables, workspaces, code objects
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():                            # alternating: every round times every variant once
                times[k].append(timed(fn, args.calls))
        assert bool(torch.isfinite(it.X).all() and torch.isfinite(it.P).all())
        best = {k: min(v) for k, v in times.items()}
        cell = lambda k: f"{best[k]:.3f} ({(max(times[k]) - best[k]) / best[k] * 100:.1f} %)"      # noqa: E731
        lines.append(f"| {name} | {lat.m} | " + " | ".join(cell(k) for k in names) +
                     f" | {best['torch'] / best['native']:.2f} | {best['torch vectors'] / best['native vectors']:.2f} |")
        print(lines[-1], flush=True)
        lat.close()
    text = (f"device: {torch.cuda.get_device_name(0)}; {VD} columns of doubles; minimum of {args.rounds} rounds of {args.calls} "
            "iterations, device events, the variants alternating; spread = (max - min) / min over the rounds\n\n"
            + "\n".join(lines) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
