"""solvers.marginal_log_likelihood(...).backward() on the GPU against tests/mll64: the composition of the native solves (fp32
lattice-row-order CG with and without the fused step forms, column padding, PCG with the fp16 factor, the caller-order
branch, K_s; float64 CG and PCG), the host-built Lanczos tridiagonals, the wide differentiable product and its backward
(plx_apply_backward, the three-call route, plx_apply_backward_f64, the torch route in double) and the ARD chain rule.

Every case is one marginal_log_likelihood + backward on a cloud of tests/lattice64.cloud at n = 257 or 701 (odd: partial
waves and workgroups; both small enough for a dense Lattice64), hyper-parameters off their defaults (mll64.set_hypers), and
asserts, from the arrays the run itself produced, recomputed in float64 (mll64.judge):
    all four gradients, every ARD entry; the true residual of every column against info["residual"]; the first moment of
    every tridiagonal, the second without a preconditioner, info["rz0"] with one; the number of tridiagonals (padding gone);
    the value identity;
and which route ran (counting wrappers, as tests/test_backward_f64_gpu.py::test_marginal_log_likelihood_gradients_agree
does).  Cases without a preconditioner add one value-only run at raw_noise = 0 whose SLQ log-determinant is compared with
the dense same-probe estimator mean_i z_i^T logm(sym(K^64)) z_i; that difference (Gauss quadrature + K's asymmetry) cannot
be derived, so the bar is mll64.LOGDET_FACTOR times what the torch formulation of the same algorithm gives on the SAME
right-hand side (the CPU path on the oracle filter; for K_s the torch loop on the dense K_s64 in the case's dtype), each
side on its full tridiagonals.  The two K_s cases alone get a derived rounding term on top (logdet_check says why).

A shape Lattice.backward_fusable refuses (fewer than 125 stacked columns: every d = 3 case below 16 columns, and 4 columns
at d = 8) takes the three-call route whatever LatticeFilterGeneral.fused_backward says; the route assertion follows the
predicate, so no case tests a fallback silently.  The worst ratio to each bar per route is printed at the end (pytest -s)
and kept in DESIGN.md."""
import copy

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import lattice_kernel as lk
from simplex_gp_amd import solvers
from tests import mll64
from tests.lattice64 import cloud

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def case(name, n, d, t, kernel="rbf1", f64=False, pre=0, steps="auto", fused_bwd=True, sym=False):
    return dict(name=name, n=n, d=d, t=t, kernel=kernel, f64=f64, pre=pre, steps=steps, fused_bwd=fused_bwd, sym=sym)


CASES = [
    # fp32, native CG: rhs 4 columns (no pad), 7 -> 8, 11 -> 12; the fused step forms on and off; d = 3 and d = 8
    case("cg-steps-t3-d3", 257, 3, 3, steps=True),
    case("cg-plain-t3-d8", 701, 8, 3, steps=False),
    case("cg-steps-t6-d8", 701, 8, 6, steps=True),
    case("cg-plain-t6-d3", 257, 3, 6, steps=False),
    case("cg-steps-t10-d8", 257, 8, 10, steps=True),
    case("cg-plain-t10-d3", 701, 3, 10, steps=False),
    # ... the three-call backward where the fused one would serve
    case("cg-staged-t6-d8", 257, 8, 6, fused_bwd=False),
    # fp32, native PCG, rank 20, fp16 factor: 7 -> 8 columns, 16 (the native limit), 17 (the caller-order branch)
    case("pcg-t6-d8", 701, 8, 6, pre=20),
    case("pcg-t15-d3", 257, 3, 15, pre=20),
    case("pcg-t16-d3", 257, 3, 16, pre=20),
    # fp32 on K_s
    case("sym-t6-d8", 257, 8, 6, sym=True),
    # Matern-1.5 order 3, d = 2: derivative taps differ from forward taps; 21 -> 24 columns
    case("matern-t20-d2", 701, 2, 20, kernel="matern32"),
    # float64
    case("f64-cg-fused", 257, 3, 4, f64=True, fused_bwd=True),
    case("f64-cg-torch", 257, 3, 4, f64=True, fused_bwd=False),
    case("f64-pcg-fused", 257, 3, 4, f64=True, pre=20, fused_bwd=True),
    case("f64-pcg-torch", 257, 3, 4, f64=True, pre=20, fused_bwd=False),
    case("f64-sym-fused", 257, 3, 4, f64=True, sym=True, fused_bwd=True),
]
IDS = [c["name"] for c in CASES]
WORST = {}            # route -> {check: worst ratio to its bar}
LOGDET = {}           # case -> (torch formulation per point, GPU per point)


class Routes:
    """Counting wrappers around the entry points that tell the routes apart; everything is put back on exit."""

    def __enter__(self):
        self.calls = {"cg_native": 0, "pcg_native": 0, "pcg_torch": 0, "cg_dtype": set(), "dot_partial": 0, "dot_full": 0,
                      "affine_sym": 0, "backward32": 0, "backward64": 0, "filter_widths": []}
        c = self.calls
        self.saved = (solvers._batched_cg_native, solvers._batched_pcg_native, solvers._batched_pcg, plx.Lattice.apply_affine,
                      plx.Lattice.apply_affine_sym_f32, plx.Lattice.apply_backward, lk.cached_filter)
        cg, pcg, pcg_t, affine, affine_sym, backward, filt = self.saved

        def cg_native(matmul, B, *a, **k):
            c["cg_native"] += 1
            c["cg_dtype"].add(B.dtype)
            return cg(matmul, B, *a, **k)

        def pcg_native(matmul, B, precond, *a, **k):
            c["pcg_native"] += 1
            c["cg_dtype"].add(B.dtype)
            c["precond"] = type(precond).__name__
            return pcg(matmul, B, precond, *a, **k)

        def pcg_torch(matmul, B, precond, *a, **k):
            c["pcg_torch"] += 1
            c["precond"] = type(precond).__name__
            return pcg_t(matmul, B, precond, *a, **k)

        def count_dot(k):
            want = k.get("want_dot", False)
            c["dot_partial"] += int(isinstance(want, str) and want == "partial")
            c["dot_full"] += int(want is True)

        def apply_affine(self_, *a, **k):
            count_dot(k)
            c["affine_sym"] += int(bool(k.get("symmetric", False)))
            return affine(self_, *a, **k)

        def apply_affine_sym_f32(self_, *a, **k):
            count_dot(k)
            c["affine_sym"] += 1
            return affine_sym(self_, *a, **k)

        def apply_backward(self_, grad_out, *a, **k):
            c["backward64" if grad_out.dtype == F64 else "backward32"] += 1
            return backward(self_, grad_out, *a, **k)

        def cached_filter(src, ref, coeffs):
            c["filter_widths"].append(int(src.shape[1]))
            return filt(src, ref, coeffs)

        solvers._batched_cg_native, solvers._batched_pcg_native, solvers._batched_pcg = cg_native, pcg_native, pcg_torch
        plx.Lattice.apply_affine, plx.Lattice.apply_affine_sym_f32 = apply_affine, apply_affine_sym_f32
        plx.Lattice.apply_backward, lk.cached_filter = apply_backward, cached_filter
        return self

    def __exit__(self, *exc):
        (solvers._batched_cg_native, solvers._batched_pcg_native, solvers._batched_pcg, plx.Lattice.apply_affine,
         plx.Lattice.apply_affine_sym_f32, plx.Lattice.apply_backward, lk.cached_filter) = self.saved
        return False


def make_model(c):
    d = c["d"]
    kernel = plx.RBFLattice(order=1, ard_num_dims=d) if c["kernel"] == "rbf1" \
        else plx.MaternLattice(nu=1.5, order=3, ard_num_dims=d)
    model = solvers.LatticeGP(kernel)
    model = (model.double() if c["f64"] else model).cuda()
    if c["sym"]:
        setattr(model, "symmetric_f64" if c["f64"] else "symmetric_f32", True)      # on the instance: nothing to restore
    return mll64.set_hypers(model)


def expected_route(c):
    """(solve route, step form, backward route) the case must take."""
    L, d = 1 + c["t"], c["d"]
    if c["f64"]:
        solve = "pcg_native" if c["pre"] else "cg_native"
        return solve, "full", "fused64" if c["fused_bwd"] else "torch64"          # (no fused step forms in double)
    if c["pre"]:
        solve = "pcg_native" if L <= 16 else "pcg_torch"
    else:
        solve = "cg_native"
    padded = L + (-L) % 4
    steps = None
    if solve != "pcg_torch":
        steps = "partial" if c["steps"] in (True, "auto") and padded in (4, 8, 12, 16) else "full"
    backward = "fused32" if c["fused_bwd"] and plx.Lattice.backward_fusable(L, d) else "staged32"
    return solve, steps, backward


def check_route(c, calls):
    solve, steps, backward = expected_route(c)
    L, d = 1 + c["t"], c["d"]
    wide = 2 * L * (1 + d)
    for name in ("cg_native", "pcg_native", "pcg_torch"):
        assert calls[name] == int(name == solve), (c["name"], "solve route", solve, calls)
    if solve != "pcg_torch":
        assert calls["cg_dtype"] == {F64 if c["f64"] else F32}, calls
    if c["pre"]:
        want = "LatticePreconditioner64" if c["f64"] else "LatticePreconditioner"
        assert calls["precond"] == want, calls
    if steps == "partial":
        assert calls["dot_partial"] > 0 and calls["dot_full"] == 0, (c["name"], "fused step forms", calls)
    elif steps == "full":
        assert calls["dot_full"] > 0 and calls["dot_partial"] == 0, (c["name"], "stand-alone step forms", calls)
    assert (calls["affine_sym"] > 0) == (c["sym"] and solve != "pcg_torch"), (c["name"], "K_s", calls)
    if backward in ("fused32", "fused64"):
        assert calls["backward32" if backward == "fused32" else "backward64"] == 1, (c["name"], backward, calls)
        assert calls["backward64" if backward == "fused32" else "backward32"] == 0 and wide not in calls["filter_widths"], calls
    else:
        assert calls["backward32"] == calls["backward64"] == 0 and calls["filter_widths"].count(wide) == 1, (c["name"], backward, calls)
    return f"{'f64' if c['f64'] else 'f32'} {solve}" + (f"/{steps}" if steps else "") + ("/K_s" if c["sym"] else "") + f" {backward}"


def torch_formulation_logdet(c, model, x32, rhs, khat, tol, max_iter):
    """The tridiagonals of the torch formulation of the same solve on the right-hand side the GPU had: the CPU path on the
    oracle filter; for K_s the torch loop on the dense K_s64 in the case's dtype."""
    if c["sym"]:
        dtype = F64 if c["f64"] else F32
        A = torch.from_numpy(khat).to(dtype)
        _, info = solvers.batched_cg(lambda V: A @ V, torch.from_numpy(rhs).to(dtype).contiguous(), max_iter=max_iter, tol=tol,
                                     want_tridiag=True)
    else:
        cpu = copy.deepcopy(model).float().cpu()
        plx.LatticeFilterGeneral.method = staticmethod(mll64.oracle_filter)
        try:
            _, info = cpu.khat_solve(torch.from_numpy(x32), torch.from_numpy(rhs).float().contiguous(), max_iter=max_iter, tol=tol,
                                     want_tridiag=True)
        finally:
            plx.LatticeFilterGeneral.method = None
    return info["tridiag"].detach().cpu().numpy().astype(np.float64)


def logdet_check(c, x32, xt, yt, tol, max_iter):
    """One value-only run at raw_noise = 0.  Returns (the torch formulation's deviation per point from the dense same-probe
    estimator, the GPU run's, the bar, the value identity's ratio to its bar for this run).  Both deviations are those of
    the FULL tridiagonals, the GPU's being the log-determinant the value identity ties to what the product returned.

    On K the bar is the issue's: LOGDET_FACTOR times the torch formulation's deviation, nothing added.  On K_s
    (symmetric_f32 / symmetric_f64) the estimator's matrix IS the operator, so the torch formulation's deviation is its own
    rounding and a multiple of it is no bar; there, and only there, a derived term is added: every CG coefficient is a
    ratio of dot products of n terms, relative error (log2 n + 4) unit (the value bar), so each tridiagonal moves by that
    much of its norm and e1^T log(T) e1 by at most that times lambda_max / lambda_min (log is 1 / lambda_min-Lipschitz on
    the spectrum), to first order."""
    n, t = c["n"], c["t"]
    model = make_model(c)
    with torch.no_grad():
        model.raw_noise.fill_(0.0)
    with mll64.capture(model) as cap, torch.no_grad():
        mll = solvers.marginal_log_likelihood(model, xt, yt, num_probes=t, cg_tol=tol, max_cg_iter=max_iter, seed=1)
    parts = mll64.value_parts64(cap, model, mll, t, symmetric=c["sym"])
    assert parts.tridiag_columns == 1 + t
    dense = mll64.dense_probe_logdet(parts.khat, cap.rhs[:, 1:])
    tri_cpu = torch_formulation_logdet(c, model, x32, cap.rhs, parts.khat, tol, max_iter)
    cpu_dev = abs(n * float(mll64.slq_terms64(tri_cpu[1:]).mean()) - dense) / n
    gpu_dev = abs(parts.logdet - dense) / n
    b = mll64.bars(n, c["d"], 1 + t, f64=c["f64"], k_fwd=0, k_bwd=0)
    bar = mll64.LOGDET_FACTOR * cpu_dev
    if c["sym"]:
        ev = np.linalg.eigvalsh(parts.khat)
        bar += b.value * float(ev[-1] / ev[0])
    lhs, rhs, scale = parts.value
    print(f"{c['name']}: log-det run, tridiagonal rows torch {tri_cpu.shape[-1]} GPU {cap.info['tridiag'].shape[-1]}, "
          f"|log-det| per point {abs(dense) / n:.3g}, bar {bar:.3g}")
    return cpu_dev, gpu_dev, bar, abs(lhs - rhs) / (b.value * scale)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        print("\nmarginal_log_likelihood on the GPU against tests/mll64, worst ratio to each bar per route:")
        for route in sorted(WORST):
            print(f"  {route}: " + "  ".join(f"{k} {v:.3g}" for k, v in sorted(WORST[route].items())))
    if LOGDET:
        print("log-det per point against the dense same-probe estimator at raw_noise = 0 (torch formulation, GPU):")
        for name, (a, b) in LOGDET.items():
            print(f"  {name}: {a:.2e} {b:.2e}")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_mll_and_gradients_against_float64(c):
    n, d, t, f64 = c["n"], c["d"], c["t"], c["f64"]
    tol, max_iter = (1e-10, 300) if f64 else (1e-4, 200)
    x32 = cloud("gauss1", n, d, seed=n + d)
    dtype = F64 if f64 else F32
    xt = torch.from_numpy(x32).to(dtype).cuda()
    yt = torch.from_numpy(mll64.targets(x32)).to(dtype).cuda()
    saved = (solvers.FUSED_CG_STEPS, plx.LatticeFilterGeneral.fused_backward, plx.LatticeFilterGeneral.fused_backward_f64)
    try:
        solvers.FUSED_CG_STEPS = c["steps"]
        if f64:
            plx.LatticeFilterGeneral.fused_backward_f64 = c["fused_bwd"]
        else:
            plx.LatticeFilterGeneral.fused_backward = c["fused_bwd"]
        plx.lattice_cache().clear()
        model = make_model(c)
        with Routes() as routes, mll64.capture(model) as cap:
            mll = solvers.marginal_log_likelihood(model, xt, yt, num_probes=t, cg_tol=tol, max_cg_iter=max_iter, seed=1,
                                                  pre_size=c["pre"])
            mll.backward()
        torch.cuda.synchronize()
        assert cap.solves == 1 and cap.products == 1 and (cap.precond is not None) == (c["pre"] > 0)
        assert mll.dtype == dtype and cap.xs_dtype == dtype
        route = check_route(c, routes.calls)
        grads = {name: p.grad.detach().cpu().numpy().copy() for name, p in model.named_parameters()}
        for name, p in model.named_parameters():
            assert p.grad.dtype == dtype, name
        ratios, parts, _ = mll64.judge(cap, model, x32, mll.detach(), grads, t, symmetric=c["sym"])
        assert parts.tridiag_columns == 1 + t, (c["name"], "the padding columns must be gone", parts.tridiag_columns)
        assert mll.cg_info["tridiag"].shape[0] == 1 + t
        if c["pre"] == 0:
            cpu_dev, gpu_dev, bar, ratios["value at raw_noise 0"] = logdet_check(c, x32, xt, yt, tol, max_iter)
            LOGDET[c["name"]] = (cpu_dev, gpu_dev)
            ratios["logdet"] = gpu_dev / bar
        w = WORST.setdefault(route, {})
        for name, r in ratios.items():
            print(f"{c['name']} [{route}]: {name} / bar {r:.3g}")
            w[name] = max(w.get(name, 0.0), r)
        bad = {k: v for k, v in ratios.items() if not v <= 1.0}
        assert not bad, (c["name"], route, bad)
    finally:
        solvers.FUSED_CG_STEPS, plx.LatticeFilterGeneral.fused_backward, plx.LatticeFilterGeneral.fused_backward_f64 = saved
        plx.LatticeFilterGeneral.method = None
        plx.lattice_cache().clear()
