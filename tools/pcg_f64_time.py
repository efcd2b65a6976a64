"""Time the float64 preconditioned solve on the native double passes next to the route a double model took before them.

Method (that of tools/cg_f64_time.py): device events around `calls` back-to-back calls, the minimum over `rounds` rounds, the
native and the parent route alternating round by round in one process on one lattice, after a warm-up of both.  Next to the
minimum the spread (max - min over the rounds, as a share of the minimum) is recorded: a difference inside it says nothing.
The factor build reads a few integers back per batch, so it is timed as one call per round between device synchronisations
(host clock).

Per shape, rank 100, 11 columns of doubles:
    apply      one preconditioner application Z = P^-1 R
                 native: LatticePreconditioner64.solve_rows (plx_pcg_project_f64 + plx_pcg_apply_f64)
                 parent: PivotedCholeskyPreconditioner(dtype=float64).solve (two GEMMs and a cholesky_solve)
    iteration  one preconditioned CG iteration
                 native: the float64 body of solvers._batched_pcg_native (plx_apply_affine_f64 with its dot,
                         plx_cg_step_update_f64, the two passes, plx_pcg_step_direction_f64)
                 parent: the body of solvers._batched_pcg on lat.apply(V).mul_(s).addcmul_(V, noise)
    build      the factor and C
                 native: the fp32 batched route + the permutation + C by plx_pcg_gram_f64
                 parent: one single-column float64 MVM per pivot
    project / apply passes alone, with their achieved bytes/s against 4 kp ld + 16 n t

    python tools/pcg_f64_time.py [--out profiles/pcg_f64_time.md] [--rounds 7] [--calls 10]

Shapes: N = 1e6, d = 8, order 1 (the headline build); N = 2e4, d = 4, order 1; the config-5 stand-in (MaternLattice nu = 1.5,
order 3, N = 10,623, d = 18).  Needs a GPU: there is no CPU timing.
"""
import argparse
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import _native as nv  # noqa: E402
from simplex_gp_amd import lattice_kernel as lk  # noqa: E402
from simplex_gp_amd import solvers  # noqa: E402

VD, RANK = 11, 100
F64 = torch.float64


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Iteration:
    """The state of a preconditioned batched CG run on (s K + noise I) X = B in double and one iteration of it per route.
    pAp is scaled up so that alpha ~ 1e-12: a few hundred timed iterations move the vectors by rounding-level amounts only."""

    def __init__(self, lat, s, noise, pre, native):
        dev, n = lat.device, lat.n_owned
        self.lat, self.n, self.pre, self.s, self.noise = lat, n, pre, s, noise
        self.ss = torch.stack([s.reshape(()), noise.reshape(())]).to(F64).contiguous()
        self.B = torch.randn(n, VD, generator=torch.Generator().manual_seed(7), dtype=F64).to(dev)
        self.X, self.R = torch.zeros_like(self.B), self.B.clone()
        self.Z = torch.empty_like(self.B)
        self.rz, self.rz_new, self.rr = (torch.ones(VD, dtype=F64, device=dev) for _ in range(3))
        if native:
            pre.solve_rows(self.R, out=self.Z, rz=self.rz)
        else:
            self.Z = pre.solve(self.R).contiguous()
            self.rz = (self.R * self.Z).sum(0)
        self.P = self.Z.clone()
        self.AP = torch.empty_like(self.B)
        self.b_norm = self.R.norm(dim=0)
        self.active = torch.ones(VD, dtype=F64, device=dev)
        self.active_next = torch.empty_like(self.active)
        self.alpha, self.beta = torch.empty_like(self.rz), torch.empty_like(self.rz)
        self.work = solvers._coldot_work(dev, VD, F64)
        self.active_b = torch.ones(VD, dtype=torch.bool, device=dev)
        self.dot_ok = lat.affine_dot_f64_ok(VD)

    def native(self):
        lib, n = nv.lib(), self.n
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.dot_ok:
            _, pap = self.lat.apply_affine(self.P, self.ss, out=self.AP, want_dot=True)
        else:
            self.lat.apply_affine(self.P, self.ss, out=self.AP)
            pap = solvers._colsum(self.P, self.AP)
        pap = (pap * 1e12).contiguous()
        nv.check(lib.plx_cg_step_update_f64(p(self.X), p(self.R), p(self.P), p(self.AP), p(self.rz), p(pap), p(self.active), n, VD,
                                            p(self.rr), p(self.alpha), p(self.work), st), "plx_cg_step_update_f64")
        self.pre.solve_rows(self.R, out=self.Z, rz=self.rz_new)
        nv.check(lib.plx_pcg_step_direction_f64(p(self.P), p(self.Z), p(self.rz_new), p(self.rz), p(self.rr), p(self.active),
                                                p(self.b_norm), 0.0, n, VD, p(self.beta), p(self.active_next), st),
                 "plx_pcg_step_direction_f64")

    def parent(self):
        X, R, P, rz, active = self.X, self.R, self.P, self.rz, self.active_b
        AP = self.lat.apply(P).mul_(self.s).addcmul_(P, self.noise).contiguous()
        pAp = solvers._colsum(P, AP) * 1e12
        alpha = torch.where(active, rz / pAp.clamp_min(1e-30), torch.zeros_like(rz))
        rr = solvers._cg_update(X, R, P, AP, alpha)
        Z = self.pre.solve(R).contiguous()
        rz_new = solvers._colsum(R, Z)
        beta = torch.where(active, rz_new / rz.clamp_min(1e-30), torch.zeros_like(rz))
        solvers._cg_direction(P, Z, beta)
        self.active_b = active & (rr.sqrt() / self.b_norm > 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcg_f64_time.py needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda", 0)
    shapes = [("N = 1e6, d = 8, order 1", 1_000_000, 8, lambda d: plx.RBFLattice(order=1, ard_num_dims=d)),
              ("N = 2e4, d = 4, order 1", 20_000, 4, lambda d: plx.RBFLattice(order=1, ard_num_dims=d)),
              ("N = 10,623, d = 18, order 3 (config-5 stand-in)", 10_623, 18,
               lambda d: plx.MaternLattice(nu=1.5, order=3, ard_num_dims=d))]
    cols = ("apply", "iteration", "build")
    lines = ["| shape | " + " | ".join(f"{c}: native ms (spread) | {c}: parent ms (spread) | parent / native" for c in cols) + " |",
             "|---|" + "---|" * (3 * len(cols))]
    passes = ["| shape | kp | ld | project ms (spread) | project GB/s | apply ms (spread) | apply GB/s |", "|---|---|---|---|---|---|---|"]
    for name, n, d, make in shapes:
        model = solvers.LatticeGP(make(d)).double().to(dev)
        x = torch.randn(n, d, generator=torch.Generator().manual_seed(1234), dtype=F64).to(dev)
        with torch.no_grad():
            ref = lk.position_hint(x.div(model.kernel.lengthscale), x, scale_of=getattr(model.kernel, "raw_lengthscale", None))
            lat = lk.lattice_cache().get(ref, model.kernel.dkernel_fn.get_coeffs())
            s, noise = model.outputscale.detach(), model.noise.detach()
            K = model.kernel(x, x)
            builds = {"native": lambda: solvers.LatticePreconditioner64(lat, s, noise, RANK),
                      "parent": lambda: solvers.PivotedCholeskyPreconditioner(K.matmul, n, s, noise, RANK, device=dev, dtype=F64)}
            pres = {k: fn() for k, fn in builds.items()}                  # warm-up of the builds, and the objects the rest uses
            its = {k: Iteration(lat, s, noise, pres[k], k == "native") for k in pres}
            Rm = its["native"].B
            Zs = {k: torch.empty_like(Rm) for k in pres}
            runs = {"apply": {"native": lambda: pres["native"].solve_rows(Rm, out=Zs["native"]),
                              "parent": lambda: pres["parent"].solve(Rm)},
                    "iteration": {"native": its["native"].native, "parent": its["parent"].parent}}
            pre = pres["native"]
            lib, st = nv.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            wk = pre._workspace(VD)
            single = {"project": lambda: nv.check(lib.plx_pcg_project_f64(p(pre._factor), pre.ld, pre.kp, p(Rm), n, VD, p(pre._cinv),
                                                                           p(pre._T), p(wk), st), "plx_pcg_project_f64"),
                      "apply": lambda: nv.check(lib.plx_pcg_apply_f64(p(pre._factor), pre.ld, pre.kp, pre.rank, p(Rm), n, VD, p(pre._T),
                                                                      p(pre._scale_solve), p(Zs["native"]), None, p(wk), st),
                                                "plx_pcg_apply_f64")}
            for group in list(runs.values()) + [single]:
                for fn in group.values():
                    for _ in range(3):
                        fn()
            torch.cuda.synchronize()
            times = {c: {k: [] for k in ("native", "parent")} for c in cols}
            ptimes = {k: [] for k in single}
            for _ in range(args.rounds):
                for c in ("apply", "iteration"):
                    for k, fn in runs[c].items():                         # alternating: every round times both routes once
                        times[c][k].append(timed(fn, args.calls))
                for k, fn in builds.items():
                    times["build"][k].append(wall(fn))
                for k, fn in single.items():
                    ptimes[k].append(timed(fn, args.calls))
            assert all(bool(torch.isfinite(i.X).all() and torch.isfinite(i.P).all()) for i in its.values())
        cell = lambda v: f"{min(v):.3f} ({(max(v) - min(v)) / min(v) * 100:.1f} %)"      # noqa: E731
        row = f"| {name} | "
        for c in cols:
            row += f"{cell(times[c]['native'])} | {cell(times[c]['parent'])} | {min(times[c]['parent']) / min(times[c]['native']):.2f} | "
        lines.append(row.rstrip())
        moved = 4 * pre.kp * pre.ld + 16 * n * VD
        passes.append(f"| {name} | {pre.kp} | {pre.ld} | {cell(ptimes['project'])} | {moved / min(ptimes['project']) / 1e6:.0f} | "
                      f"{cell(ptimes['apply'])} | {moved / min(ptimes['apply']) / 1e6:.0f} |")
        print(lines[-1], flush=True)
        print(passes[-1], flush=True)
        del pres, its, runs, single, builds, K, pre, wk, Zs, Rm
        lk.lattice_cache().clear()
        torch.cuda.empty_cache()
    text = (f"device: {torch.cuda.get_device_name(0)}; rank {RANK}, {VD} columns of doubles; minimum of {args.rounds} rounds of "
            f"{args.calls} calls, device events (the build: one call per round, host clock between synchronisations), native and "
            "parent route alternating; spread = (max - min) / min over the rounds\n\n" + "\n".join(lines) +
            "\n\nthe two passes alone; bytes/s against 4 kp ld + 16 n t\n\n" + "\n".join(passes) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
