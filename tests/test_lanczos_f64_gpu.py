"""The float64 Lanczos step (simplex_gp_amd/csrc/plx_lanczos_kernels.h with T = double) on the GPU: single steps at every
edge of plx_lanczos_shape_f64, the guard, graph replay, and the routes training.lanczos and training.PredictionCache take
for a double model.

Bars are derived, never measured.  u = 2^-53, U2 = 2^-52 = 2 u (the unit roundoff once for each side of a comparison).  A sum
of m terms in ANY order (lanes, waves, groups, the final tree; FMA or not) is off by at most m u sum|terms| to first order.
With rows = i + 1, k in {i - 1, i} and j <= i, from the values the kernel received:
    T0_k     = sum_r |Q_k[r] w[r]|                    >= |c_k|, the first coefficients; computed c_k is off by <= (n + 1) u T0_k
    a1[r]    = |w[r]| + sum_k T0_k |Q_k[r]|           >= |w1[r]| and the sum of |.| of its terms; the computed w1[r] is off by
                                                      3 u a1[r] (its own chain) + sum_k (n + 1) u T0_k |Q_k[r]| <= (n + 4) u a1[r]
    T2_j     = sum_r |Q_j[r]| a1[r]                   >= |c2_j|; computed c2_j is off by (n + 1) u T2_j (its sum) + (n + 4) u T2_j
                                                      (the error of w1 carried through) = (2 n + 5) u T2_j
    Tfull[r] = a1[r] + sum_j T2_j |Q_j[r]|            the computed w2[r] is off by (rows + 2) u Tfull[r] (its chain) +
                                                      (n + 4) u a1[r] + sum_j (2 n + 5) u T2_j |Q_j[r]| <= (2 n + rows + 7) u Tfull[r]
so  * an entry of w     2 (n + 2 rows + 16) U2 Tfull[r]      ((2 n + rows + 7) u = (n + rows / 2 + 3.5) U2: inside, with a
                                                             factor ~2 for the second-order terms and the reference's rounding)
    * alpha             2 (n + 2 rows + 16) U2 (T0_i + T2_i) ((n + 1) u T0_i + (2 n + 5) u T2_i + one addition)
    * beta^2            (n + 4) U2 sum w_dev^2, against the w the kernel stored (n squares, the sum, sqrt and its square)
    * the next vector   4 U2 |w_dev| / beta_dev per entry, against w_dev / max(beta_dev, 1e-300) (one division)
References are evaluated in np.longdouble (64-bit mantissa on x86) from the values the kernel received.  `pytest -s` prints
the worst ratio to its bar per quantity and span (report())."""
import ctypes
import math

import numpy as np
import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native as nv
from simplex_gp_amd import solvers, training
from tests.gpubuf import SENTINEL, Buf, _bits_equal, check_buffers
from tests.lattice64 import cloud
from tests.solver64 import entry_ratio

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -52
TINY64 = 1e-300
F64, F32 = torch.float64, torch.float32
LD = np.longdouble
LZ64_SYMBOLS = ("plx_lanczos_work_doubles", "plx_lanczos_shape_f64", "plx_lanczos_step_f64")
PCG64_SYMBOLS = ("plx_pcg_work_doubles", "plx_pcg_gram_f64", "plx_pcg_project_f64", "plx_pcg_apply_f64",
                 "plx_pcg_step_direction_f64")

WORST = {}
SPANS_RUN = set()


def note(what, ratio, bar):
    WORST[what] = max(WORST.get(what, 0.0), ratio / bar)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def shape(n):
    """(span, groups) of plx_lanczos_shape_f64, None where it refuses."""
    span, groups = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = nv.lib().plx_lanczos_shape_f64(n, ctypes.byref(span), ctypes.byref(groups))
    return (span.value, groups.value) if rc == 0 else None


def _last_where(pred, lo, hi):
    """The largest n in [lo, hi] with pred(n), pred monotone (true then false), pred(lo) true."""
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid - 1)
    return lo


def span_ranges():
    """[(span, first n, last n)] for every span the step uses, found by asking plx_lanczos_shape_f64."""
    top = _last_where(lambda n: shape(n) is not None, 1, 2 ** 40)
    out, first = [], 1
    while first <= top:
        span = shape(first)[0]
        last = _last_where(lambda n: shape(n)[0] == span, first, top)
        out.append((span, first, last))
        first = last + 1
    return out


# group counts whose remainder modulo 8 differs: lz_sum_groups walks the groups in four slices, two loads per trip
EXTRA_N = (509, 1277, 1533, 1789, 3069, 70_651, 77_819, 552_953, 1_073_000)


def _cases():
    try:
        if not nv.has_symbols(*LZ64_SYMBOLS):
            return [(1, 0)]
    except (ImportError, OSError):                 # (collected without a built library: the cases need its shape rule)
        return [(1, 0)]
    ranges = span_ranges()
    big = set()
    for span, first, last in ranges:
        big |= {first, last}
        if shape(last + 1) is not None:
            big.add(last + 1)
    big |= set(EXTRA_N)
    small = {1, 255, 257}
    cases = [(n, i) for n in sorted(small | {n for n in big if n <= 300}) for i in (0, 1, 2, 63, 64, 254, 255)]
    large = sorted(n for n in big if n > 300)
    cases += [(n, i) for n in large for i in (0, 3)]
    multi = min(n for n in large if shape(n)[1] > 1)
    cases.append((multi, 64))
    return cases


def test_cases_cover_every_span_and_group_tail():
    ranges = span_ranges()
    assert len(ranges) >= 1 and ranges[0][1] == 1 and ranges[-1][2] >= 2_097_152
    ns = {n for n, _ in _cases()}
    for span, first, last in ranges:
        assert {first, last} <= ns and shape(first)[0] == shape(last)[0] == span
        assert shape(last + 1) is None or (last + 1 in ns and shape(last + 1)[0] > span)
    tails = {shape(n)[1] % 8 for n in ns}
    assert {1, 2, 5, 6, 7, 12 % 8} <= tails, sorted(tails)
    assert nv.lib().plx_lanczos_work_doubles(ranges[-1][2] + 1) == -1


def ld_(a):
    return np.asarray(a, LD)


def f64_(a):
    return np.asarray(a, np.float64)


def reference(Q, w, i):
    """The step in longdouble from the doubles the kernel received, and the terms of the bars (module docstring)."""
    Ql, wl = ld_(Q[: i + 1]), ld_(w)
    Qa, wa = np.abs(Ql), np.abs(wl)
    first = max(0, i - 1)
    c0 = Ql[first:] @ wl
    T0 = np.abs(Ql[first:] * wl).sum(1)
    w1 = wl - c0 @ Ql[first:]
    a1 = wa + T0 @ Qa[first:]
    c2 = Ql @ w1
    T2 = Qa @ a1
    w2 = w1 - c2 @ Ql
    Tfull = a1 + T2 @ Qa
    return dict(w=f64_(w2), alpha=float(c0[-1] + c2[i]), Tw=f64_(Tfull), Talpha=float(T0[-1] + T2[i]))


def basis_and_w(n, i, near_span, scale=1.0, noise=1e-3):
    g = np.random.default_rng([n, i, int(near_span)])
    rows = i + 1
    M = g.standard_normal((n, rows))
    if n >= rows:
        M, _ = np.linalg.qr(M)
    else:
        M /= np.linalg.norm(M, axis=0, keepdims=True)
    Q = np.ascontiguousarray(M.T)
    del M
    w = g.standard_normal(n)
    if near_span:
        w = Q.T @ g.standard_normal(rows) * 3 + noise * w
    return Q, w * scale


def run_step(Q, w, n, i, reps=2):
    """The step on guarded buffers, `reps` times from the same inputs; checks what every case checks and returns the first
    call's (basis [rows + 1][ld], w, alpha, beta) as numpy."""
    lib = nv.lib()
    rows = i + 1
    ld = (n + 1) // 2 * 2 + (4096 if (n + i) % 2 else 0)
    basis = torch.full((rows + 1, ld), float("nan"), dtype=F64)
    basis[:rows, :n] = torch.from_numpy(Q)
    if i % 2:
        basis[rows] = SENTINEL                                 # the unused row: NaN or the sentinel
    nwork = int(lib.plx_lanczos_work_doubles(n))
    assert nwork > 0
    outs = []
    for _ in range(reps):
        QB, W = Buf(basis, dtype=F64), Buf(w, dtype=F64)
        assert QB.raw.data_ptr() % 16 == 0
        alphas, betas, work = Buf(count=256, dtype=F64), Buf(count=256, dtype=F64), Buf(count=nwork, dtype=F64)
        nv.check(lib.plx_lanczos_step_f64(QB.ptr, ld, W.ptr, n, i, alphas.ptr, betas.ptr, work.ptr, stream()), "plx_lanczos_step_f64")
        check_buffers([], [QB, W, alphas, betas, work])
        outs.append((QB.cpu(rows + 1, ld), W.cpu(), alphas.cpu(), betas.cpu()))
        del QB, W
    for other in outs[1:]:
        assert all(_bits_equal(x, y) for x, y in zip(outs[0], other)), "a repeated step differs"
    qb, wd, al, be = outs[0]
    assert _bits_equal(qb[:rows], basis[:rows]) and _bits_equal(qb[rows, n:], basis[rows, n:]), "the basis or its padding was written"
    keep = torch.ones(256, dtype=torch.bool)
    keep[i] = False
    assert torch.all(al[keep] == SENTINEL) and torch.all(be[keep] == SENTINEL), "more than entry i of alphas / betas was written"
    assert not torch.isnan(qb[rows, :n]).any() and not torch.isnan(wd).any() and math.isfinite(float(al[i])) and math.isfinite(float(be[i]))
    return qb[rows, :n].numpy(), wd.numpy(), float(al[i]), float(be[i])


def check_against_reference(Q, w, n, i, got, what):
    qn, wd, a_dev, b_dev = got
    span = shape(n)[0]
    SPANS_RUN.add(span)
    ref = reference(Q, w, i)
    bar = 2 * (n + 2 * (i + 1) + 16) * U2
    e = entry_ratio(wd, ref["w"], ref["Tw"])
    note(f"w <{span}>", e, bar)
    assert e <= bar, (what, "w", e, bar)
    e = entry_ratio(a_dev, ref["alpha"], ref["Talpha"])
    note(f"alpha <{span}>", e, bar)
    assert e <= bar, (what, "alpha", e, bar)
    ss = float((ld_(wd) * ld_(wd)).sum())
    e = entry_ratio(b_dev * b_dev, ss, ss)
    note(f"beta^2 <{span}>", e, (n + 4) * U2)
    assert e <= (n + 4) * U2, (what, "beta^2 from the stored w", e)
    div = max(b_dev, TINY64)
    e = entry_ratio(qn, f64_(ld_(wd) / LD(div)), np.abs(wd) / div)
    note(f"next vector <{span}>", e, 4 * U2)
    assert e <= 4 * U2, (what, "next vector", e)


@pytest.mark.parametrize("n,i", _cases())
@pytest.mark.parametrize("near_span", [False, True])
def test_step(n, i, near_span):
    """One step from a given basis (orthonormal in double; near_span: w lies almost in span(Q), so beta is small against
    |w|) under the bars of the module docstring; two calls bit-equal; rows 0..i and all padding untouched (NaN or the
    sentinel there: nothing may become NaN); only entry i of alphas and betas written; guards intact."""
    Q, w = basis_and_w(n, i, near_span)
    got = run_step(Q, w, n, i)
    check_against_reference(Q, w, n, i, got, f"lanczos64 n={n} i={i}{' near span' if near_span else ''}")


@pytest.mark.parametrize("n,i", [(3000, 5), (70_651, 3)])
def test_scaled_by_1e_minus_20(n, i):
    """w scaled by 1e-20: the same bars (they scale with w), alpha and beta 1e-20 times the unscaled ones to rounding, and
    no guard fires: the next vector has norm 1.  With the part of w outside span(Q) at 1e-12 of it, beta is ~1e-31 -- below
    the fp32 call's guard of 1e-30, far above this call's 1e-300."""
    Q, w = basis_and_w(n, i, False)
    _, _, a1, b1 = run_step(Q, w, n, i, reps=1)
    ws = w * 1e-20
    got = run_step(Q, ws, n, i)
    check_against_reference(Q, ws, n, i, got, f"lanczos64 scaled n={n} i={i}")
    bar = 2 * (n + 2 * (i + 1) + 16) * U2
    ref = reference(Q, w, i)
    assert abs(got[2] - 1e-20 * a1) <= 2 * bar * 1e-20 * ref["Talpha"]
    assert abs(got[3] - 1e-20 * b1) <= 2 * bar * 1e-20 * float(np.linalg.norm(ref["Tw"]))
    assert abs(float(np.linalg.norm(ld_(got[0]))) - 1.0) <= (n + 8) * U2
    Q, w = basis_and_w(n, i, True, scale=1e-20, noise=1e-12)
    got = run_step(Q, w, n, i)
    check_against_reference(Q, w, n, i, got, f"lanczos64 scaled near span n={n} i={i}")
    assert TINY64 < got[3] < 1e-30 * math.sqrt(n) and abs(float(np.linalg.norm(ld_(got[0]))) - 1.0) <= (n + 8) * U2


@pytest.mark.parametrize("n", [257, 70_651])
def test_zero_w(n):
    """w = 0 at i = 0: beta = 0, alpha = 0, row 1 all zeros (0 / 1e-300), finite."""
    Q, _ = basis_and_w(n, 0, False)
    qn, wd, a, b = run_step(Q, np.zeros(n), n, 0)
    assert a == 0.0 and b == 0.0 and not wd.any() and not qn.any()


def _one_step(lib, Qb, ld, w, n, i, alphas, betas, work, s):
    nv.check(lib.plx_lanczos_step_f64(ctypes.c_void_p(Qb.data_ptr()), ld, ctypes.c_void_p(w.data_ptr()), n, i,
                                      ctypes.c_void_p(alphas.data_ptr()), ctypes.c_void_p(betas.data_ptr()),
                                      ctypes.c_void_p(work.data_ptr()), s), "plx_lanczos_step_f64")


def test_captured_step_replays():
    """Three eager steps at n = 3000; the third once more, captured into a graph (a single chain) and replayed onto fresh
    copies of its inputs: the same bits, and the replay allocates nothing."""
    lib = nv.lib()
    n, ld = 3000, 3008
    g = torch.Generator().manual_seed(11)
    d = (1.0 + torch.rand(n, generator=g, dtype=F64)).cuda()
    Qb = torch.zeros(5, ld, dtype=F64, device="cuda")
    v0 = torch.randn(n, generator=g, dtype=F64).cuda()
    Qb[0, :n] = v0 / v0.norm()
    alphas, betas = torch.zeros(8, dtype=F64, device="cuda"), torch.zeros(8, dtype=F64, device="cuda")
    work = torch.empty(int(lib.plx_lanczos_work_doubles(n)), dtype=F64, device="cuda")
    for i in range(3):
        w = d * Qb[i, :n]
        if i == 2:
            saved = [t.clone() for t in (Qb, w, alphas, betas)]
        _one_step(lib, Qb, ld, w, n, i, alphas, betas, work, stream())
    torch.cuda.synchronize()
    eager = (Qb, w, alphas, betas)
    Q2, w2, a2, b2 = saved
    work2 = torch.empty_like(work)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _one_step(lib, Q2, ld, w2, n, 2, a2, b2, work2, ctypes.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    assert all(_bits_equal(x.cpu(), y.cpu()) for x, y in zip((Q2, w2, a2, b2), saved)), "capturing ran the step"
    before = torch.cuda.memory_allocated()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    for name, x, y in zip(("basis", "w", "alphas", "betas"), eager, (Q2, w2, a2, b2)):
        assert _bits_equal(x.cpu(), y.cpu()), name
    assert float(betas[2]) > 0 and bool((Qb[3, :n] != 0).any())


class Counter:
    """Wraps a call of the loaded library and counts."""

    def __init__(self, monkeypatch, name):
        self.calls = 0
        real = getattr(nv.lib(), name)

        def counted(*a):
            self.calls += 1
            return real(*a)

        monkeypatch.setattr(nv.lib(), name, counted)


def _double_model(d, noise=1.0, dtype=F64):
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=d))
    model = (model.double() if dtype == F64 else model).cuda()
    with torch.no_grad():
        model.raw_noise.fill_(math.log(math.expm1(noise - model.min_noise)))
    return model


def _quality(mm, Q, T):
    """(E_orth, E_rec): max |Q^T Q - I|, and max |A Q - Q T| over columns 0..t-2 relative to |alpha_0|."""
    t = Q.shape[1]
    e_orth = float((Q.t() @ Q - torch.eye(t, dtype=Q.dtype, device=Q.device)).abs().max())
    AQ = torch.cat([mm(Q[:, j:j + 1].contiguous()) for j in range(t - 1)], 1)
    e_rec = float((AQ - (Q @ T)[:, :t - 1]).abs().max() / T[0, 0].abs())
    return e_orth, e_rec


def _route_and_quality(monkeypatch, mm, v0, steps, label, leading=None):
    n = v0.shape[0]
    count = Counter(monkeypatch, "plx_lanczos_step_f64")
    Qn, Tn = training.lanczos(mm, v0, steps)
    assert count.calls == steps and Qn.dtype == F64 and tuple(Qn.shape) == (n, steps) and tuple(Tn.shape) == (steps, steps)
    monkeypatch.setattr(training, "LANCZOS_NATIVE_F64", False)
    training.lanczos(mm, v0, steps)
    assert count.calls == steps, "the switch is off"
    monkeypatch.setattr(training, "LANCZOS_NATIVE_F64", True)
    Qe, Te = training.lanczos(mm, v0, steps, graph=False, native=False)
    Qr, Tr = training._lanczos_replayed(mm, v0, steps, 32, capture=False)
    assert count.calls == steps and Qe.shape == Qn.shape and Qr.shape == Qn.shape
    floor = n * U2
    (on, rn), (oe, re_), (orr, rr) = _quality(mm, Qn, Tn), _quality(mm, Qe, Te), _quality(mm, Qr, Tr)
    print(f"{label}: E_orth native {on:.3e} eager {oe:.3e} replayed-form {orr:.3e}; E_rec native {rn:.3e} eager {re_:.3e} "
          f"replayed-form {rr:.3e}; floor {floor:.3e}")
    assert on <= 4 * max(oe, orr, floor), (label, "E_orth", on, oe, orr)
    assert rn <= 4 * max(re_, rr, floor), (label, "E_rec", rn, re_, rr)
    if leading:
        a0 = float(Te[0, 0].abs())
        spread = float((Tr[:leading, :leading] - Te[:leading, :leading]).abs().max()) / a0
        gap = float((Tn[:leading, :leading] - Te[:leading, :leading]).abs().max()) / a0
        print(f"{label}: leading {leading} x {leading} of T: native - eager {gap:.3e}, replayed-form - eager {spread:.3e} (of |alpha_0|)")
        assert gap <= 4 * max(spread, floor), (label, "T", gap, spread)


def test_lanczos_route_and_quality(monkeypatch):
    """training.lanczos on a CUDA float64 v0 takes the native step (exactly `steps` calls; none with the switch off), and
    its orthogonality and recurrence residual are within 4 x the larger of the two torch forms' (floor n U2): all three are
    rounding-level quantities of reorderings of one recurrence."""
    n, steps = 3077, 40
    g = torch.Generator().manual_seed(5)
    d = (1.0 + torch.rand(n, generator=g, dtype=F64)).cuda()
    U = torch.randn(n, 8, generator=g, dtype=F64).cuda()
    v0 = torch.randn(n, generator=g, dtype=F64).cuda()
    _route_and_quality(monkeypatch, lambda V: d.unsqueeze(-1) * V + U @ (U.t() @ V), v0, steps, "diag + rank 8, n = 3077", leading=10)
    try:
        n, steps = 2000, 30
        model = _double_model(3)
        x = torch.from_numpy(cloud("gauss1", n, 3, seed=1).astype(np.float64)).cuda()
        v0 = torch.randn(n, generator=g, dtype=F64).cuda()
        with model.khat_in_lattice_rows(x) as (mm, to_rows, from_rows):
            _route_and_quality(monkeypatch, mm, to_rows(v0.reshape(-1, 1)).squeeze(-1), steps, "double LatticeGP, n = 2000, d = 3")
    finally:
        plx.lattice_cache().clear()


@pytest.mark.parametrize("pre_size", [0, 20])
def test_prediction_cache_double_model(monkeypatch, pre_size):
    """PredictionCache of a double LatticeGP calls the native step; its variance is within 4 x the eager / replayed spread
    (floor 1e-12 max|var|) of the cache built with the switch off, its mean bit-equal (Lanczos does not enter it); a
    float32 model keeps plx_lanczos_step."""
    if pre_size and not nv.has_symbols(*PCG64_SYMBOLS):
        return
    n, d, lanc = 1500, 3, 30
    try:
        x = torch.from_numpy(cloud("gauss1", n, d, seed=4).astype(np.float64)).cuda()
        xs = torch.from_numpy(cloud("gauss1", 200, d, seed=5).astype(np.float64)).cuda()
        y = torch.sin(x.sum(1)) + 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(6), dtype=F64).cuda()
        model = _double_model(d, noise=0.1)
        c64, c32 = Counter(monkeypatch, "plx_lanczos_step_f64"), Counter(monkeypatch, "plx_lanczos_step")

        def build():
            cache = training.PredictionCache(model, x, y, cg_tol=1e-8, lanc_iter=lanc, pre_size=pre_size)
            return cache.predict(xs)

        mean_n, var_n = build()
        assert 1 <= c64.calls <= lanc and c32.calls == 0 and var_n.dtype == F64
        calls = c64.calls
        monkeypatch.setattr(training, "LANCZOS_NATIVE_F64", False)
        mean_r, var_r = build()                                  # what a double model got before: the replayed graph
        monkeypatch.setattr(training, "LANCZOS_GRAPH", False)
        mean_e, var_e = build()                                  # the eager loop
        assert c64.calls == calls and c32.calls == 0
        monkeypatch.setattr(training, "LANCZOS_GRAPH", "auto")
        monkeypatch.setattr(training, "LANCZOS_NATIVE_F64", True)
        assert torch.equal(mean_n, mean_r) and torch.equal(mean_n, mean_e)
        floor = 1e-12 * float(var_r.abs().max())
        spread = float((var_e - var_r).abs().max())
        gap = float((var_n - var_r).abs().max())
        print(f"PredictionCache double, pre_size {pre_size}: |var native - var switch-off| {gap:.3e}, eager - replayed {spread:.3e}, "
              f"floor {floor:.3e}, max|var| {float(var_r.abs().max()):.3e}")
        assert gap <= 4 * max(spread, floor), (gap, spread, floor)
        # a float32 model: the fp32 step, as before
        model32 = _double_model(d, noise=0.1, dtype=F32)
        training.PredictionCache(model32, x.float(), y.float(), cg_tol=1e-4, lanc_iter=lanc, pre_size=pre_size).predict(xs.float())
        assert c32.calls >= 1 and c64.calls == calls
    finally:
        plx.lattice_cache().clear()


def report():
    lines = ["float64 Lanczos step, worst error / derived bar per quantity and span:"]
    lines += [f"  {k}: {v:.3g}" for k, v in sorted(WORST.items())]
    return "\n".join(lines)


def test_every_span_was_run():
    """Every span of plx_lanczos_shape_f64 ran in this module (run as a whole), under its bars."""
    print(report())
    assert {s for s, _, _ in span_ranges()} <= SPANS_RUN, sorted(SPANS_RUN)
    assert all(v <= 1.0 for v in WORST.values()), WORST
