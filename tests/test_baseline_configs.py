"""BASELINE.json configs 3, 4 (all 8 shards rehearsed at full size on the one GPU; RCCL driven by one rank), 5 and the
driver's bench command line, on a real MI355X.

config 3  N=1e6, d=8, RBFLattice order 1, 50 CG iterations of the reference's training loop
          (experiments/train_simplexgp.py:29-57) at GPyTorch's default hyper-parameters
config 5  MaternLattice(nu=1.5, order=3) on the elevators stand-in (N=10,623, d=18; the UCI file is not
          redistributable, README.md:124): one MVM against the oracle and a short marginal-likelihood training run
          with the recipe of configs/simplexgp.yml:11-45
config 4  N=4e6, d=8, lengthscale 1, 8 shards: 8 local builds -> concatenated keys -> merge on every rank -> per-rank
          splat, summed accumulators (the all-reduce), blur, per-rank slice, vd in {1, 11}, against the oracle; and a
          world-size-1 "nccl" group in a child process that drives RCCL through every collective of the sharded path
bench     `python bench.py --gpus 2 ...` exactly as the driver invokes it (no launcher in the environment), two
          gloo ranks on the one GPU of the box; every rank's rows checked against the oracle
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def plx():
    import simplex_gp_amd as plx
    assert torch.cuda.is_available()
    return plx


def test_config3_full_size_cg(plx):
    """N=1e6, d=8, lengthscale = outputscale = softplus(0), noise = softplus(0) + 1e-4, right-hand side
    [y | 10 Rademacher probes]: 50 batched-CG iterations through plx_apply_affine_dot on ONE lattice build; the
    residual falls monotonically, and (sK + sigma^2 I) x_50 recomputed with the CPU oracle's filter reproduces the
    residual the HIP solve reports."""
    from simplex_gp_amd import solvers
    n, d, iters = 1_000_000, 8, 50
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=g)
    y = torch.randn(n, generator=g)
    Z = torch.randint(0, 2, (n, 10), generator=g).float() * 2 - 1
    rhs = torch.cat([y[:, None], Z], 1)
    xc, rc = x.cuda(), rhs.cuda()
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d)).cuda()
    cache = plx.lattice_cache()
    cache.clear()
    misses0 = cache.misses
    history = []
    with torch.no_grad():
        K = model.kernel(xc, xc)                    # the operator of one hyper-parameter setting: x / lengthscale + taps
        for k in (10, 25, iters):
            sol, info = model.khat_solve(xc, rc, K=K, max_iter=k, tol=0.0)
            assert info["iterations"] == k
            history.append(info["residual"].cpu().numpy())
    assert cache.misses == misses0 + 1, "one lattice build serves every CG iteration (and every solve on the same x)"
    lat = list(cache._entries.values())[-1][0]
    m_hip = lat.m
    assert "slice_vec_kernel" in lat.stage_kernels()["slice"]
    assert (history[1] < history[0]).all() and (history[2] < history[1]).all(), history
    assert history[2].max() < 5e-2          # K is only approximately symmetric (viz_mvm.ipynb:150): CG slows near 1e-2
    # the oracle's K applied to the HIP solution: one vd = 11 MVM on the host
    s, noise = float(model.outputscale), float(model.noise)
    ell = model.kernel.lengthscale.detach().cpu()
    ref = (x / ell).contiguous().numpy()
    taps = model.kernel.dkernel_fn.get_coeffs().numpy()
    sol_cpu = sol.cpu().numpy()
    oracle.set_exact_mode(False)
    try:
        Kx, m_oracle = oracle.filter(sol_cpu, ref, taps, return_m=True)
    finally:
        oracle.set_exact_mode(True)
    assert m_hip == m_oracle                       # ~1.73e6 vertices at lengthscale softplus(0)
    resid = rhs.numpy() - (s * Kx + noise * sol_cpu)
    true_rel = np.linalg.norm(resid, axis=0) / np.linalg.norm(rhs.numpy(), axis=0)
    print("config 3: HIP-reported residual", history[2], "oracle-recomputed", true_rel)
    assert np.abs(true_rel - history[2]).max() <= 1e-4
    cache.clear()


def test_config4_full_size_eight_shards(plx):
    """BASELINE.json configs[3] at full size: N = 4e6, d = 8, lengthscale 1, RBF order 1, sharded over 8 ranks, all of
    them rehearsed on the one GPU of the box: 8 x plx_build_local -> the concatenated vertex keys (what the all-gather
    delivers) -> plx_build_merge on every rank -> per-rank splat of its 5e5 rows, the accumulators summed in rank order
    (what the RCCL all-reduce delivers), blur, per-rank slice.  vd = 1 and vd = 11 ([y | 10 probes]); every rank's
    output rows against the duplicate-free oracle (<= 1e-5 rel-L2), the vertex count against the oracle's, and vd = 1
    against the oracle in the reference's exact mode (hash-growth quirk Q1 included: the north star's 1e-4)."""
    import bench
    from simplex_gp_amd.distributed import shard_bounds
    n, d, W = 4_000_000, 8, 8
    x, v = bench.synth(n, d, 11)
    taps = bench.RBF1
    lats, keys, counts = [], [], []
    for r in range(W):
        lo, hi = shard_bounds(n, W, r)
        lat = plx.Lattice()
        k = lat.build_local(x[lo:hi].contiguous().cuda(), taps)
        keys.append(k.clone())
        counts.append(int(k.shape[0]))
        lats.append(lat)
    all_keys = torch.cat(keys, 0)
    for r, lat in enumerate(lats):
        lat.build_merge(all_keys, counts, r, total_points=n)
    m = lats[0].m
    assert all(lat.m == m for lat in lats)
    xn, vn = x.numpy(), v.numpy()
    oracle.set_exact_mode(False)
    try:
        want1, m_oracle = oracle.filter(np.ascontiguousarray(vn[:, :1]), xn, taps, return_m=True)
        want11 = oracle.filter(vn, xn, taps)
    finally:
        oracle.set_exact_mode(True)
    assert m == m_oracle, (m, m_oracle)                 # 660,226 for these rows
    exact1 = oracle.filter(np.ascontiguousarray(vn[:, :1]), xn, taps)
    quirk = rel_l2(want1, exact1)
    worst = {}
    for vd, want in ((1, want1), (11, want11)):
        total = None
        for r, lat in enumerate(lats):
            lo, hi = shard_bounds(n, W, r)
            part = lat.splat(v[lo:hi, :vd].contiguous().cuda())
            total = part.clone() if total is None else total.add_(part)
        kn = lats[0].stage_kernels()
        assert ("block" in kn["splat"][0]) == (vd == 1), kn     # the shard is a coarse lattice: block tables for one column
        got = np.empty((n, vd), np.float32)
        for r, lat in enumerate(lats):
            lo, hi = shard_bounds(n, W, r)
            got[lo:hi] = lat.slice(lat.blur(total.clone(), vd=vd), vd=vd).cpu().numpy()
        worst[vd] = max(rel_l2(got[lo:hi], want[lo:hi]) for lo, hi in (shard_bounds(n, W, r) for r in range(W)))
        assert worst[vd] <= 1e-5, (vd, worst)
        if vd == 1:
            assert rel_l2(got, exact1) <= max(1e-4, quirk + 1e-5), (rel_l2(got, exact1), quirk)
            # ... and against probes of the REFERENCE's own output for these inputs (tests/golden/make_golden.py
            # --config-probes: its CPU extension run on bench.synth(4e6, 8, 11), column 0); the reference's table holds one
            # duplicate vertex here (m = 660,227: quirk Q1), the tolerance is widened by what that costs its own output
            z = np.load(os.path.join(ROOT, "tests", "golden", "filter_large.npz"))
            key = "config4_n4e6_d8_ell1.0"
            assert np.array_equal(xn[:8], z[f"{key}/ref_head"]) and np.array_equal(vn[:8, :1], z[f"{key}/src_head"])
            assert np.array_equal(exact1[:512], z[f"{key}/out_head"])             # the oracle in exact mode IS the reference
            assert 0 <= int(z[f"{key}/m"]) - m <= 12
            stride = int(z[f"{key}/stride"])
            tol = max(1e-4, quirk + 1e-5)
            assert rel_l2(got[:512], z[f"{key}/out_head"]) <= tol and rel_l2(got[::stride], z[f"{key}/out_strided"]) <= tol
            assert abs(np.linalg.norm(got.astype(np.float64)) / float(z[f"{key}/out_l2"]) - 1) <= tol
    print(f"config 4: m = {m}, worst rank rel-L2 vs oracle vd=1 {worst[1]:.2e}, vd=11 {worst[11]:.2e}; reference quirk Q1 here {quirk:.2e}")
    for lat in lats:
        lat.close()


@pytest.mark.parametrize("key", ["config4_n4e6_d8_ell1.0", "config5_n10623_d18_matern3"])
def test_config_probes_with_reference_growth_replay(plx, key):
    """The reference's own output at config 4 (N = 4e6, d = 8: its table holds one duplicate vertex, m = 660,227) and on the
    config-5 stand-in (Matern-1.5 order 3, d = 18: no duplicate, neighbours read as absent at the doublings, 4.2e-4 on its
    output) with plx_tune("reference_growth", 1): probes of the reference within 1e-4, no quirk term, and the replay's
    vertex count equal to the reference's."""
    import bench
    from simplex_gp_amd import _native as nv
    z = np.load(os.path.join(ROOT, "tests", "golden", "filter_large.npz"))
    n, d, vd = (int(v) for v in z[f"{key}/shape"])
    if key.startswith("config4"):
        x, v = bench.synth(n, d, 11)
        v = v[:, :1].contiguous()
    else:
        g = torch.Generator().manual_seed(int(z[f"{key}/seed"]))
        x = torch.randn(n, d, generator=g)
        v = torch.randn(n, 1, generator=g)
    ref = (x / float(z[f"{key}/ell"])).contiguous()
    assert np.array_equal(ref[:8].numpy(), z[f"{key}/ref_head"]) and np.array_equal(v[:8].numpy(), z[f"{key}/src_head"])
    nv.check(nv.lib().plx_tune(b"reference_growth", 1), "plx_tune")
    try:
        lat = plx.Lattice().build(ref.cuda(), z[f"{key}/taps"])
        out = lat.apply(v.cuda()).cpu().numpy()
        info = lat.reference_growth_info()
    finally:
        nv.check(nv.lib().plx_tune(b"reference_growth", 0), "plx_tune")
    print(key, info)
    assert info["replayed"] and not info["inexact"] and info["m_reference"] == int(z[f"{key}/m"])
    stride = int(z[f"{key}/stride"])
    assert rel_l2(out[:512], z[f"{key}/out_head"]) <= 1e-4
    assert rel_l2(out[::stride], z[f"{key}/out_strided"]) <= 1e-4
    assert abs(np.linalg.norm(out.astype(np.float64)) / float(z[f"{key}/out_l2"]) - 1) <= 1e-4
    assert abs(float(out.astype(np.float64).sum()) - float(z[f"{key}/out_sum"])) <= 1e-4 * float(z[f"{key}/out_abs_sum"])
    lat.close()


def test_rccl_world_size_one():
    """RCCL on real hardware: a child process opens a world-size-1 "nccl" process group (device_id=...) and runs the
    sharded path with its collectives forced on -- key all-gather, vertex all-reduce, CG dot-product all-reduce, barrier
    with device_ids -- bit for bit against the plain lattice (tests/checks/rccl_world1.py)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "rccl_world1.py")], env=env,
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "RCCL_WORLD1_OK" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-3000:]
    print(proc.stdout)


def test_config5_matern_order3_d18(plx):
    """Stand-in for UCI elevators: one MVM vs the oracle (m = 201,837: every corner its own vertex), then marginal-
    likelihood training (Adam lr 0.1, cg_tol 1, 10 probes, min_noise 0.1: configs/simplexgp.yml) with a finite,
    falling -MLL."""
    from simplex_gp_amd import solvers, training
    n, d = 10623, 18
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(n, d, generator=g)
    y = torch.sin(x[:, 0]) + 0.5 * torch.cos(x[:, 1] * x[:, 2]) + 0.1 * torch.randn(n, generator=g)
    v = torch.randn(n, 1, generator=g)
    k = plx.MaternLattice(nu=1.5, order=3, ard_num_dims=d)
    taps = k.dkernel_fn.get_coeffs().numpy()
    assert taps.shape == (7,)
    lat = plx.Lattice().build(x.cuda(), taps)
    out = lat.apply(v.cuda()).cpu().numpy()
    oracle.set_exact_mode(False)
    try:
        want, m = oracle.filter(v.numpy(), x.numpy(), taps, return_m=True)
    finally:
        oracle.set_exact_mode(True)
    assert lat.m == m == 201_837
    assert rel_l2(out, want) <= 1e-5
    # the same operator against probes of the REFERENCE's own output (make_golden.py --config-probes: x, v drawn as
    # SURVEY 8d draws them, x first then v from one generator seeded 1234; the reference builds the same 201,837 vertices)
    z = np.load(os.path.join(ROOT, "tests", "golden", "filter_large.npz"))
    key = "config5_n10623_d18_matern3"
    g2 = torch.Generator().manual_seed(int(z[f"{key}/seed"]))
    x2 = torch.randn(n, d, generator=g2)
    v2 = torch.randn(n, 1, generator=g2)
    assert np.array_equal(x2[:8].numpy(), z[f"{key}/ref_head"]) and np.array_equal(v2[:8].numpy(), z[f"{key}/src_head"])
    assert np.allclose(taps, z[f"{key}/taps"], atol=1e-6) and int(z[f"{key}/m"]) == lat.m
    got2 = lat.apply(v2.cuda()).cpu().numpy() if torch.equal(x2, x) else plx.Lattice().build(x2.cuda(), z[f"{key}/taps"]).apply(v2.cuda()).cpu().numpy()
    stride = int(z[f"{key}/stride"])
    # the oracle in exact mode reproduces the reference's probes bit for bit; the HIP output is 1e-5 from the duplicate-free
    # oracle and as far from the reference as the reference's own quirk Q1 puts it (here no duplicate vertex, but
    # neighbours read as absent at the table doublings: measured on this very input, never a literal)
    exact2 = oracle.filter(v2.numpy(), x2.numpy(), z[f"{key}/taps"])
    assert np.array_equal(exact2[:512], z[f"{key}/out_head"]) and np.array_equal(exact2[::stride], z[f"{key}/out_strided"])
    oracle.set_exact_mode(False)
    try:
        clean2 = oracle.filter(v2.numpy(), x2.numpy(), z[f"{key}/taps"])
    finally:
        oracle.set_exact_mode(True)
    quirk = rel_l2(clean2, exact2)
    print("config 5: reference quirk Q1 on this input", quirk, "HIP vs reference", rel_l2(got2, exact2))
    assert rel_l2(got2, clean2) <= 1e-5
    assert rel_l2(got2, exact2) <= max(1e-4, quirk + 1e-5)
    assert abs(np.linalg.norm(got2.astype(np.float64)) / float(z[f"{key}/out_l2"]) - 1) <= max(1e-4, quirk + 1e-5)
    lat.close()
    model = solvers.LatticeGP(k, min_noise=0.1).cuda()
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    history, _ = training.fit(model, (x.cuda(), y.cuda()), epochs=100, lr=0.1, num_probes=10, cg_iter=500, cg_tol=1.0,
                              pre_size=100)          # the recipe of configs/simplexgp.yml, all of its 100 epochs (round 6; 12 before)
    torch.cuda.synchronize()
    mll = np.array([h["train/mll"] for h in history])
    print("config 5 stand-in: 100 epochs in %.2f s; train/mll every 10th epoch" % (time.perf_counter() - t0), np.round(mll[::10], 4),
          "last", round(float(mll[-1]), 4), "lengthscale range", float(model.kernel.lengthscale.detach().min()), float(model.kernel.lengthscale.detach().max()))
    assert len(mll) == 100 and np.isfinite(mll).all()
    assert mll[:12][-3:].mean() > mll[:3].mean() + 0.01    # -MLL falls from the start (the round-5 assertion on the first 12 epochs)
    assert mll[-10:].mean() > mll[:3].mean() + 0.05         # ... and keeps the ground it gained over the whole run
    assert (np.diff(mll) > -0.1).all()                       # no epoch undoes the progress (probe noise and Adam's overshoot only)


def test_evaluation_and_the_next_step_share_lattice_and_preconditioner(plx):
    """The reference's loop (train_simplexgp.py:123-165): step, evaluate on two splits, step ...  Between an evaluation
    and the next step the optimiser does not move, so (1) both splits predict from ONE mean / variance cache
    (training.PredictionCache: GPyTorch's eval-mode prediction strategy), (2) the next step's operator -- the same data under
    the same lengthscale, as a new tensor -- is served the evaluation's lattice without a build, (3) and its
    preconditioner.  'Same' is decided on the parameters' VALUES (fused Adam writes them without moving their version
    counters): after an optimiser step nothing is taken for the same.  Values equal those computed with nothing remembered."""
    from simplex_gp_amd import solvers, training
    torch.manual_seed(0)
    n, d = 6000, 5
    x = torch.randn(n, d).cuda()
    y = (torch.sin(x[:, 0]) + 0.1 * torch.randn(n, device="cuda"))
    xv, xt = torch.randn(500, d).cuda(), torch.randn(700, d).cuda()
    model = solvers.LatticeGP(plx.MaternLattice(nu=1.5, order=2, ard_num_dims=d), min_noise=0.1).cuda()
    opt = training.make_optimizer(model, lr=0.1)
    cache = plx.lattice_cache()
    cache.clear()

    def step(seed):
        opt.zero_grad()
        mll = solvers.marginal_log_likelihood(model, x, y, num_probes=10, max_cg_iter=500, cg_tol=1.0, seed=seed, pre_size=50)
        (-mll).backward()
        return float(mll), {k: p.grad.clone() for k, p in model.named_parameters()}

    step(0)
    versions = {k: p._version for k, p in model.named_parameters()}
    opt.step()
    print("version counters moved by the optimiser:", {k: p._version > versions[k] for k, p in model.named_parameters()})
    same0, reuse0 = cache.same_positions, model.__dict__.get("preconditioner_reuses", 0)
    pc = training.PredictionCache(model, x, y, cg_tol=1e-2, lanc_iter=50, pre_size=50)
    mv, vv = pc.predict(xv)
    mt, vt = pc.predict(xt)
    for xs, m_c, v_c in ((xv, mv, vv), (xt, mt, vt)):                          # the shared cache predicts what predict() alone does
        m_1, v_1 = training.predict(model, x, y, xs, cg_tol=1e-2, lanc_iter=50, pre_size=50)
        assert torch.allclose(m_c, m_1, atol=2e-4, rtol=1e-3) and torch.allclose(v_c, v_1, atol=2e-4, rtol=1e-3)
    misses = cache.misses
    reuse1 = model.preconditioner_reuses                                        # (the predict() calls above reused it too)
    got, got_grads = step(1)
    assert cache.same_positions > same0 and model.preconditioner_reuses == reuse1 + 1 > reuse0
    assert cache.misses - misses <= 1                                           # at most the lattice of the derivative taps
    # nothing remembered: the same value and gradients
    cache.clear()
    model.__dict__.pop("_last_preconditioner")
    want, want_grads = step(1)
    assert abs(got - want) <= 1e-4 * max(1.0, abs(want))
    for k in got_grads:
        assert torch.allclose(got_grads[k], want_grads[k], rtol=2e-3, atol=1e-5), k
    # ... and after the optimiser moved, nothing is taken for the same
    opt.step()
    reuse2, same2 = model.preconditioner_reuses, cache.same_positions
    step(2)
    assert model.preconditioner_reuses == reuse2 and cache.same_positions == same2


@pytest.mark.parametrize("n,steps", [(3000, 40), (777, 256), (70_001, 48), (300_000, 33), (1_200_003, 24)])
def test_lanczos_native_step_equals_the_torch_recurrence(plx, n, steps):
    """plx_lanczos_step (four launches per step: two Gram-Schmidt passes, coefficients, next basis vector) against the
    three-term torch loop, on a symmetric operator cheap enough for every row-span shape of the kernels (256 / 1024 /
    4096 / 8192 rows per workgroup) and for the full 256 basis rows: the same T and leading basis vectors to fp32 Lanczos
    accuracy, Q orthonormal, Q^T A Q = T, bit-identical when repeated; shapes the library does not serve take the torch form."""
    from simplex_gp_amd import training
    g = torch.Generator().manual_seed(n)
    dvec = (1.0 + 3.0 * torch.rand(n, generator=g)).cuda()
    U = (torch.randn(n, 3, generator=g) / n ** 0.5).cuda()
    v0 = torch.randn(n, generator=g).cuda()

    def mm(V):
        return dvec[:, None] * V + U @ (U.T @ V)
    Q0, T0 = training.lanczos(mm, v0, steps, graph=False)
    Q1, T1 = training.lanczos(mm, v0, steps)
    assert training.LANCZOS_NATIVE and Q1.shape == Q0.shape == (n, steps) and T1.shape == T0.shape
    scale = float(T0.diagonal().abs().max())
    k = min(steps, 12)
    assert float((T1[:k, :k] - T0[:k, :k]).abs().max()) <= 1e-4 * scale
    assert float((Q1[:, :6] - Q0[:, :6]).abs().max()) <= 1e-4
    eye = torch.eye(steps, device="cuda")
    assert float((Q1.T @ Q1 - eye).abs().max()) <= 1e-4
    assert float((Q1.T @ mm(Q1.contiguous()) - T1).abs().max()) <= 2e-4 * scale
    Q2, T2 = training.lanczos(mm, v0, steps)
    assert torch.equal(T1, T2) and torch.equal(Q1, Q2)
    if n == 3000:
        # a Krylov space exhausted after 4 vectors: the same cut as the torch loop; more steps than the library's 256 rows:
        # the torch form serves
        low = lambda V: V + U @ (U.T @ V)                                      # noqa: E731
        Qa, Ta = training.lanczos(low, v0, 40, graph=False)
        Qb, Tb = training.lanczos(low, v0, 40)
        assert Qa.shape == Qb.shape and Qb.shape[1] <= 5 and float((Ta - Tb).abs().max()) <= 1e-4
        Qc, Tc = training.lanczos(mm, v0, 300)
        assert Qc.shape[1] <= 300 and float((Tc[:8, :8] - T0[:8, :8]).abs().max()) <= 1e-4 * scale


def test_lanczos_replayed_graph_equals_the_eager_loop(plx):
    """training.lanczos on the GPU replays ONE captured step (HIP graph, step index on the device) on the operator in
    lattice row order: the same tridiagonal and basis as the eager three-term loop on the caller-order operator, to fp32
    Lanczos accuracy; an operator that cannot be captured (it reads the device back) falls back to the eager loop, leaves
    the reason in _graph_refusals, and the next capture works."""
    from simplex_gp_amd import solvers, training
    torch.manual_seed(0)
    n, d, steps = 3000, 6, 40
    x = torch.randn(n, d).cuda()
    r = torch.randn(n).cuda()
    model = solvers.LatticeGP(plx.MaternLattice(nu=1.5, order=2, ard_num_dims=d), min_noise=0.1).cuda()
    with torch.no_grad():
        mm = model.khat_matmul(x)
        Q0, T0 = training.lanczos(mm, r, steps, graph=False)
        with model.khat_in_lattice_rows(x) as (mm_rows, to_rows, from_rows):
            Q1, T1 = training.lanczos(mm_rows, to_rows(r.reshape(-1, 1)).squeeze(-1), steps, graph=True)   # True: a refusal raises
            Q1 = from_rows(Q1.contiguous())
        assert Q1.shape == Q0.shape == (n, steps) and T1.shape == T0.shape
        scale = float(T0.diagonal().abs().max())
        assert float((T1 - T0).abs().max()) <= 2e-3 * scale
        assert float((Q1[:, :8] - Q0[:, :8]).abs().max()) <= 1e-3                  # the leading vectors agree; later ones
        A_Q = torch.cat([mm(Q1[:, j:j + 1].contiguous()) for j in range(steps)], 1)  # drift apart as any two fp32 Lanczos runs do,
        H = Q1.T @ A_Q                                                               # but diagonal and sub-diagonal of Q^T A Q
        assert float((H.diagonal() - T1.diagonal()).abs().max()) <= 2e-3 * scale     # are T's for each (the lattice operator is
        assert float((H.diagonal(-1) - T1.diagonal(-1)).abs().max()) <= 2e-3 * scale  # only approximately symmetric: the upper
        assert float(H.tril(-2).abs().max()) <= 2e-3 * scale                         # triangle is not T's)
        assert float((Q1.T @ Q1 - torch.eye(steps, device="cuda")).abs().max()) <= 1e-4
        # a refused capture: the eager loop's answer, and the library is usable afterwards
        training._graph_refusals.clear()
        calls = []

        def reads_back(V):
            out = mm(V)
            calls.append(float(out[0, 0]))                                         # a host read-back: not capturable
            return out
        Q2, T2 = training.lanczos(reads_back, r, steps, native=False)
        assert len(training._graph_refusals) == 1 and T2.shape == T0.shape
        assert float((T2 - T0).abs().max()) <= 2e-3 * scale
        Q3, T3 = training.lanczos(mm, r, steps, graph=True)
        assert float((T3 - T0).abs().max()) <= 2e-3 * scale


def test_predict_matches_dense_formulas_on_gpu(plx):
    """training.predict on the HIP path (CG mean + Lanczos variance through the rectangular operator, py:142-160)
    against the dense expressions built from the same operators, n = 2000."""
    from simplex_gp_amd import solvers, training
    torch.manual_seed(0)
    n, ns = 2000, 300
    x = (torch.rand(n, 2) * 4).cuda()
    y = (torch.sin(2 * x[:, 0]) * torch.cos(x[:, 1]) + 0.1 * torch.randn(n, device="cuda"))
    xs = (torch.rand(ns, 2) * 4).cuda()
    model = solvers.LatticeGP(plx.RBFLattice(order=1), min_noise=1e-2).cuda()
    mean, var = training.predict(model, x, y, xs, cg_tol=1e-7, lanc_iter=400)
    with torch.no_grad():
        s, noise = model.outputscale.double(), model.noise.double()
        K = model.kernel(x, x).evaluate().double()
        Ks = model.kernel(xs, x).evaluate().double()              # [ns, n]
        Khat = s * K + noise * torch.eye(n, device="cuda", dtype=torch.float64)
        r = (y - model.mean).reshape(-1, 1).double()
        mean_dense = model.mean.double() + (s * Ks @ torch.linalg.solve(Khat, r)).squeeze(-1)
        var_dense = s - ((s * Ks) * torch.linalg.solve(Khat, (s * Ks).T).T).sum(1)
    assert mean.shape == (ns,) and var.shape == (ns,)
    # the lattice operator is only approximately symmetric (viz_mvm.ipynb:150): CG / Lanczos see its action
    assert rel_l2(mean.cpu().numpy(), mean_dense.cpu().numpy()) <= 2e-2
    assert (var > 0).all()
    assert float((var.double() - var_dense.clamp_min(1e-8)).abs().max()) <= 0.05 * float(s)
    # and against the ORACLE's operators: K(x, x) and K(xs, x) column by column through the CPU restatement's filter
    # (py:133-134 square; py:150-156 rectangular = one square filter over the stacked points [x; xs], rows of xs), then
    # the dense predictive mean -- nothing of the HIP path in this reference value
    ell = model.kernel.lengthscale.detach().cpu()
    taps = model.kernel.dkernel_fn.get_coeffs().numpy()
    xo, xso = (x.cpu() / ell).numpy(), (xs.cpu() / ell).numpy()
    oracle.set_exact_mode(False)
    try:
        K_o = oracle.filter(np.eye(n, dtype=np.float32), xo, taps)
        stacked = np.concatenate([xo, xso], 0)
        rhs = np.concatenate([np.eye(n, dtype=np.float32), np.zeros((ns, n), np.float32)], 0)
        Ks_o = oracle.filter(rhs, stacked, taps)[n:]                              # [ns, n]
    finally:
        oracle.set_exact_mode(True)
    assert rel_l2(K.cpu().numpy(), K_o) <= 1e-5 and rel_l2(Ks.cpu().numpy(), Ks_o) <= 1e-5
    sd, nd = float(s), float(noise)
    Khat_o = sd * K_o.astype(np.float64) + nd * np.eye(n)
    mean_o = float(model.mean) + sd * Ks_o.astype(np.float64) @ np.linalg.solve(Khat_o, r.cpu().numpy())
    assert rel_l2(mean.cpu().numpy(), mean_o[:, 0]) <= 2e-2


def test_lengthscale_gradient_vs_central_differences(plx):
    """d/d(raw lengthscale) of v^T K v / n by autograd against central finite differences of the same lattice
    operator, smooth v.  The reference's position gradient (py:113-123) carries the factor -2 of the profile
    exp(-d^2) it differentiates, while the filter it is applied through realises exp(-d^2 / 2) (permutohedral
    embedding scale, h:372-390): the autograd gradient is therefore TWICE the finite-difference slope of the operator
    (reference quirk Q2 in DESIGN.md; the mirror reproduces the reference's gradients to 2e-5, test_autograd_*).
    Checked here: sign, and magnitude = 2 x slope within 8 % (measured 1.02 - 1.06 on the CPU oracle)."""
    torch.manual_seed(1)
    n = 20000
    k = plx.RBFLattice(order=1).cuda()
    x = torch.randn(n, 2, device="cuda")
    v = (torch.sin(2 * x[:, 0]) + torch.cos(x[:, 1]))[:, None].contiguous()

    def q():
        return (v * k(x, x).matmul(v)).sum() / n
    q().backward()
    g = k.raw_lengthscale.grad.item()
    raw0 = k.raw_lengthscale.detach().clone()
    h = 3e-2
    with torch.no_grad():
        k.raw_lengthscale.copy_(raw0 + h)
        qp = q().item()
        k.raw_lengthscale.copy_(raw0 - h)
        qm = q().item()
        k.raw_lengthscale.copy_(raw0)
    fd = (qp - qm) / (2 * h)
    print("lengthscale gradient: autograd", g, "central difference", fd, "ratio", g / fd)
    assert fd != 0 and np.sign(g) == np.sign(fd)
    assert abs(g / (2 * fd) - 1) <= 0.08


def test_bench_self_launches_its_ranks(tmp_path):
    """`python bench.py --gpus 2 --steps K --warmup W` with no launcher in the environment (the driver's command for
    N > 1 without torchrun): bench.py starts torch.distributed.run as a child, the ranks build the lattice from
    their own rows (local build, key all-gather, merge), one JSON line comes back on stdout, exit code 0, and every
    rank's output rows match the CPU oracle."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dump = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--points", "30000",
           "--rebuild-every", "2", "--backend", "gloo", "--skip-configs", "--dump", dump, "--scaling", "weak", "--full"]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["rccl_ranks"] == 2 and res["steps"] == 4 and res["scaling"] == "weak"
    assert res["config"]["n_total"] == 60000 and res["config"]["builds_in_timed_region"] == 2
    assert res["value"] > 0 and res["value"] == res["mvms_per_s"]          # the plain rate, never scaled by the size
    assert res["allreduce_bytes"] == res["config"]["m_vertices"] * 4
    assert set(res["stage_us"]) == {"splat", "exchange", "blur", "slice"}
    assert res["exchange"]["bytes"] == res["allreduce_bytes"] and res["exchange"]["us"] > 0 and "all_reduce" in res["exchange"]["kind"]
    # the prediction beside the measurement: what the rank's own stage times say two GPUs are worth against one
    exp = res["expected_speedup_vs_1gpu"]
    st = res["stage_us"]
    assert abs(exp["t_rank_us"] - sum(st.values())) < 0.5
    assert abs(exp["t_one_gpu_us"] - (2 * (st["splat"] + st["slice"]) + st["blur"])) < 0.5
    assert 0 < exp["warm_mvm"] <= 2.0 + 1e-6 and exp["warm_mvm"] <= exp["warm_mvm_if_exchange_were_free"]
    assert "with_one_build_per_2_mvms" in exp and "6x" in res["expected_speedup_note"]
    check = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "check_bench_dump.py"), dump], env=env,
                           capture_output=True, text=True, timeout=600)
    assert check.returncode == 0 and "OK" in check.stdout, check.stdout + check.stderr
    # the default: strong scaling, BASELINE.json's metric as written -- same total size whatever the rank count
    cmd2 = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--points", "30000",
            "--backend", "gloo", "--skip-configs"]
    proc2 = subprocess.run(cmd2, env=env, capture_output=True, text=True, timeout=900)
    assert proc2.returncode == 0, proc2.stderr[-3000:]
    res2 = json.loads([ln for ln in proc2.stdout.splitlines() if ln.startswith("{")][0])
    assert res2["config"]["n_total"] == 30000 and res2["scaling"] == "strong" and res2["value"] == res2["mvms_per_s"]
    # a launcher whose world size disagrees with --gpus is an error, not a silently different job
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="1", RANK="0"),
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2


def test_bench_multi_rank_full_legs_rehearsal():
    """The driver's multi-GPU command with EVERY leg -- `python bench.py --gpus N --steps 20 --warmup 5 --full` -- rehearsed with
    N = 4 gloo ranks on the one GPU (the GPU boxes admit at most 6 processes on a card, so the 8-rank command itself cannot
    be rehearsed here; nothing in bench.py depends on the rank count beyond the shard bounds), the fixed-size legs shrunk
    through PLX_BENCH_CONFIG4_POINTS.  One JSON line, rc 0, every leg present with its exchange record
    {kind, bytes, us}, wall seconds per leg, the build's key all-gather timed."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PLX_BENCH_CONFIG4_POINTS"] = "200000"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "20", "--warmup", "5", "--points", "100000",
           "--backend", "gloo", "--full"]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 4 and res["rccl_ranks"] == 4 and res["steps"] == 20 and res["warmup"] == 5
    assert res["value"] > 0 and res["scaling"] == "strong"

    def is_exchange(e):
        return isinstance(e, dict) and {"kind", "bytes", "us"} <= set(e) and e["us"] >= 0 and e["bytes"] >= 0
    assert is_exchange(res["exchange"])
    assert is_exchange(res["build_key_allgather"]) and res["build_key_allgather"]["bytes"] > 0 and res["build_key_allgather"]["us"] > 0
    for leg in ("config4", "weak_1e6_per_gpu", "weak_4e6_per_gpu"):
        assert leg in res, leg
        assert is_exchange(res[leg]["exchange_vd1"]), leg
        assert res[leg]["mvms_per_s_vd1"] > 0
    assert is_exchange(res["config4"]["exchange_vd11"])
    assert 0 < res["expected_speedup_vs_1gpu"]["warm_mvm"] <= 4.0 + 1e-6
    for leg, vd in (("config4", 1), ("config4", 11), ("weak_1e6_per_gpu", 1), ("weak_4e6_per_gpu", 1)):
        e = res[leg][f"expected_speedup_vs_1gpu_vd{vd}"]
        assert 0 < e["warm_mvm"] <= 4.0 + 1e-6 and 0 <= e["replicated_share_of_rank_time"] <= 1, (leg, vd, e)
    assert "columns_mode" in res and "config3_cg" in res and "grid_vd11" in res["config4"]
    for mode in ("points", "columns"):
        assert is_exchange(res["config3_cg"][mode]["exchange"]), mode
    walls = res["leg_wall_s"]
    for leg in ("main", "config4", "weak_1e6_per_gpu", "weak_4e6_per_gpu", "columns_mode", "config3_cg", "config4_grid_vd11"):
        assert leg in walls and walls[leg] >= 0, leg
    assert res["total_wall_s"] < 600                       # the driver's limit for the real run
    print("leg_wall_s", walls, "total", res["total_wall_s"])


def test_bench_single_rank_rccl_rehearsal():
    """bench.py's own multi-rank code path on real RCCL: PLX_BENCH_SINGLE_RANK_RCCL=1 makes the one-GPU run open a
    world-size-1 "nccl" group (init with device_id, barrier with device_ids, all_reduce of the timings on the device,
    sharded build with its key all-gather, MVMs with the vertex all-reduce) and report like a multi-GPU job."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PLX_BENCH_SINGLE_RANK_RCCL"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--points", "200000", "--skip-configs",
           "--full"]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-3000:]
    res = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][0])
    assert res["n_gpus"] == 1 and res["rccl_ranks"] == 1 and res["backend"] == "nccl" and res["value"] > 0
    assert res["exchange"]["bytes"] == res["config"]["m_vertices"] * 4 and res["exchange"]["us"] > 0
    assert res["build_key_bytes_exchanged"] > 0


def test_bench_single_gpu_json_contract():
    """`python bench.py --steps K --warmup W --full` (the driver's N = 1 command with every leg): ONE JSON line with the contract keys, the
    roofline object of the dominant stage (algorithmic bytes over a launch time measured in this run, PMC traffic from
    the committed profile) and the CPU baseline of the reference path on this host."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "10", "--warmup", "2", "--skip-configs", "--skip-fine",
           "--full"]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    res = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in res, key
    assert res["n_gpus"] == 1 and res["steps"] == 10 and res["warmup"] == 2 and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["data"] == "synthetic" and res["vs_baseline"] is None
    assert "workload" in res["config"] and "model" not in res["config"]
    assert res["value"] > 0 and abs(res["value"] * res["ms_per_step"] / 1e3 - 1.0) < 0.02      # value = steps / time
    roof = res["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3 and 0.0 < roof["frac"] < 1.0
    assert abs(roof["achieved"] - roof["bytes_per_launch"] / (roof["launch_us"] * 1e-6) / 1e9) < 0.02 * roof["achieved"]
    assert roof["traffic"] is None or roof["traffic"] > 0.5 * roof["bytes_per_launch"]
    cpu = res["cpu_baseline"]
    assert cpu["kind"] in ("reference", "port") and cpu["cores"] == 1 and cpu["value"] > 0 and cpu["sample"]
    assert res["config"]["builds_in_timed_region"] == 1


def test_bench_plain_run_headline_and_outputs(tmp_path):
    """A plain `python bench.py --steps K --warmup W --dump-outputs DIR`: ONE JSON line with the headline keys only (no leg
    of --full), `ms_per_step` the time of one of the K timed steps, and DIR/out.npy the MVM output of the last timed step,
    which matches the CPU oracle on the same seeded inputs; a second run with the same arguments writes the same output,
    and two gloo ranks on the one GPU write the same rows of the same operator (gathered in row order)."""
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    n, d, ell = 100_000, 8, 1.0
    outs = []
    for run, ranks in enumerate(("1", "1", "2")):
        dump = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", ranks, "--steps", "7", "--warmup", "2",
               "--points", str(n), "--rebuild-every", "3", "--dump-outputs", str(dump)] + (["--backend", "gloo"] if ranks == "2" else [])
        proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0, proc.stderr[-3000:]
        lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, proc.stdout
        res = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"):
            assert key in res, key
        for key in ("roofline", "stages", "fine", "cpu_baseline", "config3", "config4", "warm_mvms_per_s"):
            assert key not in res, key
        assert res["steps"] == 7 and res["warmup"] == 2 and res["config"]["builds_in_timed_region"] == 3
        assert res["unit"] == "MVMs/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
        assert res["ms_per_step"] > 0 and abs(res["value"] * res["ms_per_step"] / 1e3 - 1.0) < 0.02
        assert sorted(os.listdir(dump)) == ["out.npy"]
        out = np.load(dump / "out.npy")
        assert out.dtype == np.float32 and out.shape == (n, 1)
        outs.append(out)
    x, v = bench.synth(n, d, 1)
    oracle.set_exact_mode(False)
    try:
        want = oracle.filter(v.numpy(), (x / ell).numpy(), bench.RBF1)
    finally:
        oracle.set_exact_mode(True)
    assert rel_l2(outs[0], want) <= 1e-5 and rel_l2(outs[2], want) <= 1e-5
    assert rel_l2(outs[1], outs[0]) <= 1e-6


def test_bench_train_step_phases_add_up(plx):
    """bench.py's training-step leg: the reported phases (median of three profiled steps) add up to the synchronised step
    they were taken from within 25 %, and the un-synchronised step_ms is not above it (round 4 reported an `optimizer` phase
    of 73 ms inside a 12.8 ms step: one outlier step)."""
    import bench
    from simplex_gp_amd import solvers
    solvers.cap_host_threads()          # as bench.main does: the process-wide BLAS-pool cap is the caller's opt-in (the
                                        # library only caps the pool inside its own small host factorisations)

    class Ctx:
        dev = torch.device("cuda:0")

        @staticmethod
        def sync():
            torch.cuda.synchronize()

    out = bench.train_step_leg(Ctx, 200_000, 6, lambda: plx.RBFLattice(order=1, ard_num_dims=6), pre_sizes=(0, 100), steps=3)
    for key in ("pre_size_0", "pre_size_100"):
        leg = out[key]
        assert leg["phases_from"].startswith("median")
        assert abs(leg["phases_sum_ms"] - leg["profiled_step_ms"]) <= 0.25 * leg["profiled_step_ms"], leg
        assert leg["step_ms"] <= 1.6 * leg["profiled_step_ms"], leg      # (host-bound at this size: generous)
        assert all(v >= 0 for v in leg["phases_ms"].values())


def test_cg_iteration_launch_counts(plx):
    """A plain CG iteration of khat_solve at 12 columns, d = 8: splat + fix-up, four two-axis blur passes + one single pass,
    slice, update, direction = 10 kernel launches when the column reductions run inside the update and the direction kernels
    (round 6; what solvers does by itself up to FUSED_CG_MAX_ROWS rows, where an iteration is launch-bound), 12 with the two
    stand-alone reductions (above that: measured neutral to 0.5 % slower at N >= 1e5, tools/ab_cg_steps_r6.py).  Counted from
    HIP-graph captures of a 6- and a 2-iteration solve (bench.cg_launch_leg, the bench line's
    `config3.launches_per_cg_iteration`); the device is usable afterwards."""
    import bench
    from simplex_gp_amd import solvers

    class Ctx:
        dev = torch.device("cuda:0")

    assert solvers.FUSED_CG_STEPS == "auto"
    small = bench.cg_launch_leg(Ctx, n=50_000, d=8)
    large = bench.cg_launch_leg(Ctx, n=150_000, d=8)
    assert small is not None and large is not None, "the CG iteration could not be captured into a HIP graph"
    assert small["kernels"] == small["graph_nodes"] == 10.0, small
    assert large["kernels"] == large["graph_nodes"] == 12.0, large
    assert float(torch.ones(8, device="cuda").sum()) == 8.0


@pytest.mark.parametrize("name,n,d", [("houseelectric (10 % of its rows)", 204_928, 11), ("precipitation", 628_474, 3),
                                      ("keggdirected", 48_827, 20), ("elevators", 16_599, 17), ("protein", 45_730, 9)])
def test_published_shapes_against_the_oracle(plx, name, n, d):
    """The (n, d) of the reference's published MVM timings (notebooks/viz_compute.ipynb:102-106) on synthetic standardised
    clouds, lengthscale softplus(0): one MVM against the oracle (vertex count and output), d = 11, 17 and 20 at sizes where
    every kernel family runs whole grids.  houseelectric's full 2,049,280 x 11 takes the oracle three minutes on one host
    core: it is checked at full size by tests/checks/published_shapes_check.py (1.1e-6 in round 4) and here on a tenth of its rows."""
    import bench
    g = torch.Generator().manual_seed(1234)
    ref = (torch.randn(n, d, generator=g) / 0.6931).contiguous()
    v = torch.randn(n, 1, generator=g)
    lat = plx.Lattice().build(ref.cuda(), bench.RBF1)
    out = lat.apply(v.cuda())
    oracle.set_exact_mode(False)
    try:
        want, m = oracle.filter(v.numpy(), ref.numpy(), bench.RBF1, return_m=True)
    finally:
        oracle.set_exact_mode(True)
    assert lat.m == m, (name, lat.m, m)
    assert rel_l2(out.cpu().numpy(), want) <= 1e-5, name
    # the one-shot boundary call (what the reference's filter() is) gives the same operator
    once = plx.filter(v.cuda(), ref.cuda(), torch.from_numpy(bench.RBF1))
    assert rel_l2(once.cpu().numpy(), want) <= 1e-5, name
    lat.close()
