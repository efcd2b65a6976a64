"""TEST HELPER: solvers.marginal_log_likelihood recomputed in float64 from the arrays one run of it produced.

The surrogate whose gradient marginal_log_likelihood hands to autograd is

    S = -u^T r + 1/2 u^T (K^ V)[:, 0] - 1/(2t) sum_i w_i^T (K^ V)[:, i],    K^ = s K(x / l) + sigma^2 I,   V = [u | Z']

with u, W = sol[:, :1], sol[:, 1:] detached and Z' the probes (P^-1 Z with a preconditioner).  Given sol, V and the scaled
positions x~ = x / l, its gradient in every hyper-parameter is an explicit expression; with G = [u/2 | -W/(2t)]:

    dS/d mean = sum(u)        dS/d s = sum(G * K64 V)        dS/d sigma^2 = sum(G * V)
    dS/d x~   = s * backward64(G, V, x~, derivative taps).grad_x

K64 = tests/lattice64.Lattice64 (forward taps).  The lengthscale gradient is dS/d x~ pulled back through
x / softplus(raw_lengthscale) by torch autograd in float64, the outputscale and noise gradients pick up sigmoid(raw), and
everything is divided by n.  capture() reads sol, V, the right-hand side and the scaled positions off one run by wrapping
three methods on the model INSTANCE; no product code changes.  Nothing here compares a stochastic estimate with its
expectation or depends on how far CG converged: every number is a deterministic function of the captured arrays.

Each gradient comes with a yardstick, the sum of the absolute values of the terms it adds up (times the same chain factor),
so that an error is judged in units of what the entry sums:
    lengthscale j   Y_j = s sigmoid(raw_l_j) / n * sum_p T[p, j] |x[p, j]| / l_j^2,   T from lattice64.contract64
                    (float64 models: T' of tests/test_backward_f64_gpu.py, the bar of that file being stated against it)
    outputscale     sigmoid(raw_s) / n * sum(|G| * terms64(V))
    noise, mean     sigmoid(raw_noise) / n * sum |G * V|,   sum |u| / n

value_parts64() does the same for the value: the true residual of every column against K^64, the first two moments that the
first row of each Lanczos tridiagonal must equal (algebraic consequences of the CG recurrence; they hold for the
non-symmetric K),
    T_i[0, 0] = p^T K^ p / b^T p,  p = b (plain) or P^-1 b (preconditioned);   T_i[0, 0]^2 + T_i[0, 1]^2 = |K^ b|^2 / |b|^2 (plain)
the SLQ log-determinant recomputed with numpy.linalg.eigh from cg_info["tridiag"][1:], and the identity
    n * mll = -quad / 2 - logdet_SLQ / 2 - n / 2 log 2 pi,      quad = sum(r * u).

Bars (bars()): nothing measured on the code under test.  (The one bar that IS measured, at run time and on the torch
formulation, not on the code under test, is the log-determinant's against the dense same-probe estimator:
tests/test_mll_gpu.py::logdet_check, LOGDET_FACTOR below.)
    fp32   TAU = 7e-7 and REL = 3.5e-6 of tests/test_backward_fp64.py (grad_x against its terms, forward product), and the
           reduction term RED = (log2(n d L) + 4) 2^-24 for the fp32 sums of the chain rule:
           lengthscale (TAU + RED) Y_j, outputscale (REL + RED) Y, noise and mean RED Y, moments relative 2 REL + RED,
           value relative (log2 n + 4) 2^-24 of |quad| / 2 + |logdet| / 2, residual 1e-4 (test_config3_full_size_cg)
    fp64   the same construction with 2 (k + 4 (L + 1)) 2^-52 (tests/test_backward_f64_gpu.py, k the depth of the
           derivative-tap lattice) for TAU, k 2^-52 (tests/test_f64_gpu.py, forward-tap lattice) for REL, 2^-53 for 2^-24,
           residual 1e-10 (tests/test_cg_f64_gpu.py)
Where a yardstick is 0 the value must be exactly 0 (lattice64.entry_ratio's rule); no entry is left out.

Checker only: the product never imports it.
"""
import contextlib
import math
import types

import numpy as np
import torch

from oracle import oracle
from tests.lattice64 import Lattice64, backward64, entry_ratio, stack64
from tests.test_backward_fp64 import REL, TAU

RAW_OUTPUTSCALE, RAW_NOISE, MEAN = 0.3, -1.0, 0.2        # off the defaults: no factor is 1
LOGDET_FACTOR = 4.0                                    # GPU log-det bar = this x the torch formulation's own deviation


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def oracle_filter(src, ref, coeffs):
    """The CPU oracle as LatticeFilterGeneral.method, on the duplicate-free lattice (the one the HIP build and Lattice64
    have)."""
    oracle.set_exact_mode(False)
    try:
        out = oracle.filter(src.detach().numpy(), ref.detach().numpy(), coeffs.detach().numpy())
    finally:
        oracle.set_exact_mode(True)
    return torch.from_numpy(out)


def set_hypers(model):
    """The hyper-parameters of every case: no factor 1, no two ARD dimensions alike."""
    with torch.no_grad():
        raw = model.kernel.raw_lengthscale
        raw.copy_(torch.linspace(-0.3, 0.4, raw.numel(), dtype=raw.dtype).reshape(raw.shape) if raw.numel() > 1
                  else torch.full_like(raw, -0.3))
        model.raw_outputscale.fill_(RAW_OUTPUTSCALE)
        model.raw_noise.fill_(RAW_NOISE)
        model.mean.fill_(MEAN)
    return model


def targets(x, seed=3):
    """y for the cloud x (float64 numpy [n])."""
    rng = np.random.default_rng(seed)
    return np.sin(np.asarray(x, np.float64).sum(1)) + 0.1 * rng.standard_normal(x.shape[0])


@contextlib.contextmanager
def capture(model):
    """with capture(model) as cap: one marginal_log_likelihood(model, ...) inside leaves in cap
        rhs [n, 1 + t], sol, info        what khat_solve was given and returned
        V, KV                            the argument and the result of the one differentiable product
        precond, pinv_r                  the preconditioner (or None) and precond.solve(rhs[:, :1]), the first direction of column 0
        xs                               the scaled positions the operator was built on, read back from the device
    as float64 numpy arrays (info and precond as they are).  Three wrappers on the instance, removed on exit."""
    cap = types.SimpleNamespace(rhs=None, sol=None, info=None, V=None, KV=None, precond=None, pinv_r=None, xs=None,
                                xs_dtype=None, solves=0, products=0)
    solve, matmul, make_pre = model.khat_solve, model.khat_matmul, model.preconditioner
    state = {"solving": False}

    def khat_solve(x, rhs, K=None, **kw):
        state["solving"] = True
        try:
            sol, info = solve(x, rhs, K=K, **kw)
        finally:
            state["solving"] = False
        xs = K.x if K is not None and hasattr(K, "x") else x.div(model.kernel.lengthscale)
        cap.rhs, cap.sol, cap.info, cap.xs = _np(rhs), _np(sol), info, _np(xs)
        cap.xs_dtype = xs.dtype
        pre = kw.get("precond")
        if pre is not None:
            cap.pinv_r = _np(pre.solve(rhs.contiguous())[:, :1])
        cap.solves += 1
        return sol, info

    def khat_matmul(x, K=None):
        mm = matmul(x, K)
        if state["solving"]:                 # (the CPU path's solve asks for the same closure: not the product we are after)
            return mm

        def product(V):
            out = mm(V)
            cap.V, cap.KV = _np(V), _np(out)
            cap.products += 1
            return out
        return product

    def preconditioner(*a, **kw):
        cap.precond = make_pre(*a, **kw)
        return cap.precond

    model.khat_solve, model.khat_matmul, model.preconditioner = khat_solve, khat_matmul, preconditioner
    try:
        yield cap
    finally:
        for name in ("khat_solve", "khat_matmul", "preconditioner"):
            delattr(model, name)


def _softplus(a):
    return np.logaddexp(0.0, a)


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def hypers64(model):
    """(s, sigma^2, l [d or 1], raw_s, raw_noise, raw_l) in float64 from the raw parameters."""
    raw_s, raw_n = float(model.raw_outputscale.detach()), float(model.raw_noise.detach())
    raw_l = _np(model.kernel.raw_lengthscale).reshape(-1)
    return types.SimpleNamespace(s=float(_softplus(raw_s)), noise=float(_softplus(raw_n)) + float(model.min_noise),
                                 l=_softplus(raw_l), raw_s=raw_s, raw_n=raw_n, raw_l=raw_l)


class Operators64:
    """The forward-tap and derivative-tap Lattice64 of one captured run, built once and shared by the gradient and the
    value recomputation."""

    def __init__(self, cap, model):
        dk = model.kernel.dkernel_fn
        self.taps = np.asarray(dk.get_coeffs().detach().cpu().numpy(), np.float32)
        self.dtaps = np.asarray(dk.get_deriv_coeffs().detach().cpu().numpy(), np.float32)
        self.xs = cap.xs
        self._fwd = self._bwd = None

    @property
    def fwd(self):
        if self._fwd is None:
            self._fwd = Lattice64(self.xs, self.taps)
        return self._fwd

    @property
    def bwd(self):
        if self._bwd is None:
            self._bwd = Lattice64(self.xs, self.dtaps)
        return self._bwd

    @staticmethod
    def depth(l64):
        """k of tests/test_f64_gpu.py from the float64 structure: the longest vertex row, the taps on each axis, the
        slice's corners, the division and slack."""
        lmax = int(np.diff(l64.S.tocsc().indptr).max())
        r = l64.coeffs.size // 2
        return lmax + (2 * r + 1) * (l64.d + 1) + 2 * (l64.d + 1) + 8


def _terms_T(G, V, xs, l64):
    """T' of tests/test_backward_f64_gpu.py: contract64's T with every filtered entry replaced by the size of its terms."""
    n, L = G.shape
    d = xs.shape[1]
    t = l64.terms64(stack64(G, V, xs))
    tg, tgx, ts, tsx = np.split(t, [L, L + L * d, 2 * L + L * d], axis=1)
    tgx, tsx = tgx.reshape(n, L, d), tsx.reshape(n, L, d)
    a3, b3, y3 = np.abs(V)[:, :, None], np.abs(G)[:, :, None], np.abs(xs)[:, None, :]
    return 2.0 * (a3 * y3 * tg[:, :, None] + a3 * tgx + b3 * y3 * ts[:, :, None] + b3 * tsx).sum(1)


def surrogate_grads64(cap, model, x, num_probes, ops=None, terms_yardstick=False):
    """{parameter name: (gradient of the marginal likelihood's surrogate in float64, its yardstick)} for the four
    hyper-parameters, shaped like the parameters, from the captured run.  x: the positions the model was given (any
    float array); terms_yardstick: T' instead of T for the lengthscale (the float64 bars are stated against it)."""
    ops = ops if ops is not None else Operators64(cap, model)
    h = hypers64(model)
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float64)
    n, t = cap.sol.shape[0], int(num_probes)
    assert cap.sol.shape == cap.V.shape == cap.rhs.shape == (n, 1 + t)
    u, W, V = cap.sol[:, :1], cap.sol[:, 1:], cap.V
    G = np.concatenate([u / 2.0, -W / (2.0 * t)], axis=1)
    out = {"mean": (np.float64(u.sum() / n), np.float64(np.abs(u).sum() / n))}
    KV = ops.fwd.apply(V)
    c = _sigmoid(h.raw_s) / n
    out["raw_outputscale"] = (np.float64(c * (G * KV).sum()), np.float64(c * (np.abs(G) * ops.fwd.terms64(V)).sum()))
    c = _sigmoid(h.raw_n) / n
    out["raw_noise"] = (np.float64(c * (G * V).sum()), np.float64(c * np.abs(G * V).sum()))
    gx, _, T = backward64(G, V, ops.xs, ops.dtaps, lattice=ops.bwd)
    if terms_yardstick:
        T = _terms_T(G, V, ops.xs, ops.bwd)
    raw = torch.tensor(h.raw_l.reshape(model.kernel.raw_lengthscale.shape), dtype=torch.float64, requires_grad=True)
    scaled = torch.from_numpy(x) / torch.nn.functional.softplus(raw)
    (scaled * torch.from_numpy(h.s * gx)).sum().backward()
    want = raw.grad.numpy() / n
    Y = h.s * _sigmoid(h.raw_l) / n * (T * np.abs(x)).sum(0) / h.l ** 2          # [d]; one shared lengthscale: broadcast
    Y = Y.reshape(want.shape) if want.size == Y.size else np.full(want.shape, Y.sum())
    out["kernel.raw_lengthscale"] = (want, Y)
    return out


def slq_terms64(tridiag):
    """e1^T log(T_i) e1 per column with numpy.linalg.eigh."""
    tri = np.asarray(tridiag.detach().cpu().numpy() if torch.is_tensor(tridiag) else tridiag, np.float64)
    ev, evec = np.linalg.eigh(tri)
    return (evec[:, 0, :] ** 2 * np.log(np.maximum(ev, 1e-30))).sum(-1)


def khat64(ops, h, symmetric=False):
    K = ops.fwd.matrix()
    if symmetric:
        K = 0.5 * (K + K.T)
    return h.s * K + h.noise * np.eye(K.shape[0])


def value_parts64(cap, model, mll, num_probes, ops=None, symmetric=False):
    """What the value side of one captured run must satisfy, recomputed in float64 (symmetric: the solve ran on
    K_s = (K + K^T) / 2).  Returns a namespace of (got, want) pairs -- residual, moment1, moment2 (None with a
    preconditioner or a single iteration), weights (preconditioner only) -- and logdet (SLQ recomputed), quad, and the
    value identity as (n * mll, -quad/2 - logdet/2 - n/2 log 2 pi, |quad|/2 + |logdet|/2)."""
    ops = ops if ops is not None else Operators64(cap, model)
    h = hypers64(model)
    n = cap.rhs.shape[0]
    A = khat64(ops, h, symmetric)
    info = cap.info
    tri = _np(info.get("tridiag_host", info["tridiag"]))
    B, X = cap.rhs, cap.sol
    out = types.SimpleNamespace(tridiag_columns=tri.shape[0], khat=A)
    bn = np.linalg.norm(B, axis=0)
    out.residual = (_np(info["residual"]), np.linalg.norm(B - A @ X, axis=0) / bn)
    if cap.precond is None:
        AB = A @ B
        out.moment1 = (tri[:, 0, 0], (B * AB).sum(0) / (B * B).sum(0))
        out.moment2 = (tri[:, 0, 0] ** 2 + tri[:, 0, 1] ** 2, (AB * AB).sum(0) / (B * B).sum(0)) if tri.shape[-1] > 1 else None
        out.weights = None
        terms = slq_terms64(tri[1:])
        out.logdet = float(n) * float(terms.mean())
    else:
        Pb = np.concatenate([cap.pinv_r, cap.V[:, 1:]], axis=1)            # P^-1 b per column: V[:, 1:] = P^-1 Z
        w = (B * Pb).sum(0)
        out.moment1 = (tri[:, 0, 0], (Pb * (A @ Pb)).sum(0) / w)
        out.moment2 = None
        rz0 = _np(info["rz0"])
        out.weights = (rz0, w)
        out.logdet = float(cap.precond.logdet()) + float((rz0[1:] * slq_terms64(tri[1:])).mean())
    out.quad = float((B[:, 0] * X[:, 0]).sum())
    want = -0.5 * out.quad - 0.5 * out.logdet - 0.5 * n * math.log(2.0 * math.pi)
    out.value = (float(n) * float(mll), want, 0.5 * abs(out.quad) + 0.5 * abs(out.logdet))
    return out


def dense_probe_logdet(A, Z):
    """mean_i z_i^T logm(sym(A)) z_i: the estimator SLQ approximates, on the same probes."""
    ev, Q = np.linalg.eigh(0.5 * (A + A.T))
    QZ = Q.T @ np.asarray(Z, np.float64)
    return float(((QZ * QZ) * np.log(ev)[:, None]).sum(0).mean())


def bars(n, d, L, f64=False, k_fwd=None, k_bwd=None):
    """The bars of the module docstring for one shape."""
    unit = 2.0 ** -53 if f64 else 2.0 ** -24
    red = (math.log2(n * d * L) + 4.0) * unit
    if f64:
        tau, rel = 2.0 * (k_bwd + 4.0 * (L + 1)) * 2.0 ** -52, k_fwd * 2.0 ** -52
    else:
        tau, rel = TAU, REL
    return types.SimpleNamespace(lengthscale=tau + red, outputscale=rel + red, noise=red, mean=red, moment=2.0 * rel + red,
                                 value=(math.log2(n) + 4.0) * unit, residual=1e-10 if f64 else 1e-4)


def rel_ratio(got, want, bar):
    """max |got - want| / (bar |want|) over every entry; where want = 0, got must be exactly 0."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    return entry_ratio(got, want, np.abs(want)) / bar


def lengthscale_ratio(cap, model, x, num_probes, got):
    """The lengthscale gradient autograd left (`got`) against the float64 one of the captured fp32 run: worst
    |error| / (bar x yardstick) over its entries, <= 1 passes."""
    n, d, L = cap.rhs.shape[0], cap.xs.shape[1], cap.rhs.shape[1]
    want, Y = surrogate_grads64(cap, model, x, num_probes)["kernel.raw_lengthscale"]
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64).reshape(want.shape)
    return entry_ratio(got, want, Y) / bars(n, d, L).lengthscale


def judge(cap, model, x, mll, grads, num_probes, symmetric=False):
    """Every ratio to its bar for one captured run: {name: worst |error| / bar}, <= 1 passes.  grads: {parameter name:
    array} as autograd left them.  Also returns the value parts (for the log-det comparison) and the operators."""
    f64 = cap.xs_dtype == torch.float64
    ops = Operators64(cap, model)
    n, d, L = cap.rhs.shape[0], cap.xs.shape[1], cap.rhs.shape[1]
    k_fwd, k_bwd = (ops.depth(ops.fwd), ops.depth(ops.bwd)) if f64 else (None, None)
    b = bars(n, d, L, f64=f64, k_fwd=k_fwd, k_bwd=k_bwd)
    want = surrogate_grads64(cap, model, x, num_probes, ops=ops, terms_yardstick=f64)
    assert set(want) == set(grads), (sorted(want), sorted(grads))
    ratios = {}
    for name, bar in (("mean", b.mean), ("raw_outputscale", b.outputscale), ("raw_noise", b.noise),
                      ("kernel.raw_lengthscale", b.lengthscale)):
        w, Y = want[name]
        got = np.asarray(grads[name], np.float64).reshape(np.shape(w))
        ratios["grad " + name] = entry_ratio(got, w, Y) / bar
    parts = value_parts64(cap, model, mll, num_probes, ops=ops, symmetric=symmetric)
    got, true = parts.residual
    ratios["residual"] = float(np.abs(got - true).max()) / b.residual
    ratios["moment1"] = rel_ratio(*parts.moment1, b.moment)
    if parts.moment2 is not None:
        ratios["moment2"] = rel_ratio(*parts.moment2, b.moment)
    if parts.weights is not None:
        ratios["weights"] = rel_ratio(parts.weights[0][1:], parts.weights[1][1:], b.moment)
    lhs, rhs, scale = parts.value
    ratios["value"] = abs(lhs - rhs) / (b.value * scale)
    return ratios, parts, ops
