"""The exact kernel MVM on the GPU (plx_exact_mvm / plx_exact_grad through simplex_gp_amd.exact) against fp64 torch on
the GPU, evaluated from the same fp32 inputs: forward for every profile over the shape / d / t grid (with and without a
large common offset), far and coincident points, determinism (split j range included), gradients, the kernel classes,
the lattice's exact twin and one large call."""
import math

import pytest
import torch

import simplex_gp_amd as plx

pytestmark = pytest.mark.gpu

DEV = "cuda"
PROFILES = ["rbf", "matern12", "matern32", "matern52"]


def k64(d2, profile):
    """The profile in fp64, a differentiable function of d2 (r = 0 handled so that the r = 0 convention falls out)."""
    if profile == "rbf":
        return torch.exp(-d2)
    r = torch.sqrt(d2 + 1e-300)
    if profile == "matern12":
        return torch.exp(-r)
    if profile == "matern32":
        s = math.sqrt(3) * r
        return (1 + s) * torch.exp(-s)
    s = math.sqrt(5) * r
    return (1 + s + 5.0 / 3.0 * d2) * torch.exp(-s)


def dense64(x1, x2, v, profile):
    """K(x1, x2) @ v in fp64 by direct differences, in blocks of at most 2^25 differences."""
    a, b, w = x1.detach().double(), x2.detach().double(), v.detach().double()
    cj = max(1, min(b.shape[0], (1 << 25) // (256 * a.shape[1])))
    out = []
    for i in range(0, a.shape[0], 256):
        acc = 0
        for j in range(0, b.shape[0], cj):
            d2 = ((a[i:i + 256, None, :] - b[None, j:j + cj, :]) ** 2).sum(-1)
            acc = acc + k64(d2, profile) @ w[j:j + cj]
        out.append(acc)
    return torch.cat(out)


def dense64_diff(x1, x2, v, profile):
    """The same, differentiable in all three (pairwise differences materialised: small sizes only)."""
    d2 = ((x1[:, None, :] - x2[None, :, :]) ** 2).sum(-1)
    return k64(d2, profile) @ v


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def points(n, d, seed, spread=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * (spread / math.sqrt(d))).to(DEV)


def values(n, t, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(n, t, generator=g).to(DEV)


# (n1, n2, d, t): square n = 1 ... 4096, the rectangular shapes, every d and t of the grid
SHAPES = [(1, 1, 1, 1), (2, 2, 3, 3), (129, 129, 8, 11), (1000, 1000, 18, 64), (4096, 4096, 3, 1), (4096, 4096, 32, 3),
          (300, 300, 1, 257), (1, 5000, 8, 1), (777, 3001, 3, 11), (3001, 777, 18, 257), (640, 640, 32, 64)]


@pytest.mark.parametrize("offset", [0.0, 30.0])
@pytest.mark.parametrize("profile", PROFILES)
def test_forward_against_fp64(profile, offset):
    for n1, n2, d, t in SHAPES:
        x2 = points(n2, d, 1) + offset
        x1 = x2 if n1 == n2 else points(n1, d, 2) + offset
        v = values(n2, t, 3)
        out = plx.exact_matmul(x1, x2, v, profile)
        assert out.shape == (n1, t) and out.dtype == torch.float32
        err = rel_l2(out, dense64(x1, x2, v, profile))
        assert err <= 1e-5, (profile, offset, n1, n2, d, t, err)


def test_vector_rhs_and_noncontiguous_inputs():
    x = points(700, 5, 4)
    v = values(700, 2, 5)
    want = dense64(x, x, v, "rbf")
    assert rel_l2(plx.exact_matmul(x, x, v[:, 0], "rbf"), want[:, 0]) <= 1e-5
    xt = x.t().contiguous().t()                                   # a transposed view: not contiguous
    assert rel_l2(plx.exact_matmul(xt, xt, v, "rbf"), want) <= 1e-5


@pytest.mark.parametrize("profile", PROFILES)
def test_far_and_coincident_points(profile):
    # far apart: k underflows to 0 off the diagonal, K = I
    n, d = 300, 4
    x = (torch.arange(n, dtype=torch.float32)[:, None] * 100.0).repeat(1, d).to(DEV)
    v = values(n, 3, 6)
    x.requires_grad_(True)
    vv = v.clone().requires_grad_(True)
    out = plx.exact_matmul(x, x, vv, profile)
    assert torch.isfinite(out).all() and rel_l2(out.detach(), v) <= 1e-6
    out.square().sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) == 0.0
    assert torch.isfinite(vv.grad).all()
    # coincident: K = ones, every pair at r = 0
    y = torch.full((257, 3), 1.25, device=DEV, requires_grad=True)
    w = values(257, 2, 7)
    out = plx.exact_matmul(y, y, w, profile)
    assert rel_l2(out.detach(), w.sum(0, keepdim=True).expand(257, 2)) <= 1e-6
    out.sum().backward()
    assert torch.isfinite(y.grad).all() and float(y.grad.abs().max()) == 0.0


@pytest.mark.parametrize("n1,n2,t", [(8, 200_000, 1), (8, 200_000, 11), (3000, 3000, 3)])
def test_deterministic(n1, n2, t):
    x2 = points(n2, 8, 8)
    x1 = points(n1, 8, 9)
    v = values(n2, t, 10)
    a = plx.exact_matmul(x1, x2, v, "matern32")
    b = plx.exact_matmul(x1, x2, v, "matern32")
    assert torch.equal(a, b)
    g = values(n1, t, 11)
    from simplex_gp_amd.exact import _grad
    assert torch.equal(_grad(x1, x2, g, v, 2), _grad(x1, x2, g, v, 2))
    if n1 == 8:
        assert rel_l2(a, dense64(x1, x2, v, "matern32")) <= 1e-5


def _check_grads(profile, x1, x2, v, square):
    G = values(x1.shape[0], v.shape[1], 12)
    a1 = x1.clone().requires_grad_(True)
    a2 = a1 if square else x2.clone().requires_grad_(True)
    av = v.clone().requires_grad_(True)
    (plx.exact_matmul(a1, a2, av, profile) * G).sum().backward()
    b1 = x1.double().requires_grad_(True)
    b2 = b1 if square else x2.double().requires_grad_(True)
    bv = v.double().requires_grad_(True)
    (dense64_diff(b1, b2, bv, profile) * G.double()).sum().backward()
    got = [(a1.grad, b1.grad), (av.grad, bv.grad)] + ([] if square else [(a2.grad, b2.grad)])
    for name, (mine, want) in zip(["x1", "v", "x2"], got):
        assert torch.isfinite(mine).all(), (profile, name)
        err = rel_l2(mine, want)
        assert err <= 1e-4, (profile, square, name, err)


@pytest.mark.parametrize("profile", PROFILES)
def test_gradients_against_fp64_autograd(profile):
    x = points(300, 3, 13)
    _check_grads(profile, x, x, values(300, 2, 14), square=True)
    _check_grads(profile, points(200, 5, 15), points(333, 5, 16), values(333, 3, 17), square=False)
    _check_grads(profile, points(150, 18, 18), points(170, 18, 19), values(170, 20, 20), square=False)   # t > 16: blocks


def test_matern12_duplicated_points():
    y = points(100, 3, 21)
    x = torch.cat([y, y, y[:10]])                        # every point at least twice: pairs at r = 0 off the diagonal
    v = values(x.shape[0], 2, 22)
    _check_grads("matern12", x, x, v, square=True)
    _check_grads("matern12", x, y, values(100, 2, 23), square=False)


@pytest.mark.parametrize("make,profile", [(lambda d: plx.RBFExact(ard_num_dims=d), "rbf"),
                                          (lambda d: plx.MaternExact(nu=2.5, ard_num_dims=d), "matern52"),
                                          (lambda d: plx.MaternExact(nu=0.5), "matern12")])
def test_kernel_classes(make, profile):
    d = 4
    k = make(d).to(DEV)
    ls = torch.tensor([[0.7, 1.1, 0.9, 1.4]])[:, :k.raw_lengthscale.shape[-1]]
    k.lengthscale = ls.to(DEV)
    x, xs = points(900, d, 24), points(130, d, 25)
    V = values(900, 3, 26)
    lsd = k.lengthscale.detach().double()
    K = k(x, x)
    assert isinstance(K, plx.ExactLazyKernel) and tuple(K.shape) == (900, 900)
    assert torch.equal(K.diag(), torch.ones(900, device=DEV))
    assert torch.equal(k(x, x, diag=True), torch.ones(900, device=DEV))
    assert rel_l2(K @ V, dense64(x.double() / lsd, x.double() / lsd, V, profile)) <= 1e-5
    Ks = k(xs, x)
    assert tuple(Ks.shape) == (130, 900)
    assert rel_l2(Ks @ V, dense64(xs.double() / lsd, x.double() / lsd, V, profile)) <= 1e-5
    W = values(130, 3, 27)
    assert rel_l2(Ks.t() @ W, dense64(x.double() / lsd, xs.double() / lsd, W, profile)) <= 1e-5
    # the lengthscale gradient, through the position gradients of both operands
    k.zero_grad()
    ((K @ V).square().sum() + (Ks @ V * values(130, 3, 28)).sum()).backward()
    raw = k.raw_lengthscale.detach().double().clone().requires_grad_(True)
    l64 = torch.nn.functional.softplus(raw)
    xd, xsd = x.double() / l64, xs.double() / l64
    loss = dense64_diff(xd, xd, V.double(), profile).square().sum() \
        + (dense64_diff(xsd, xd, V.double(), profile) * values(130, 3, 28).double()).sum()
    loss.backward()
    assert rel_l2(k.raw_lengthscale.grad, raw.grad) <= 1e-4


def test_exact_twin_against_the_lattice():
    n, d = 5000, 3
    x = points(n, d, 29, spread=1.5 * math.sqrt(d))
    w = torch.tensor([[0.7], [-0.4], [0.3]], device=DEV)
    v = torch.sin(x @ w) + 0.5                           # smooth in the positions
    lat = plx.RBFLattice(order=1).to(DEV)
    lat.lengthscale = 1.0
    twin = plx.exact_twin(lat)
    assert twin.profile == "rbf" and torch.allclose(twin.lengthscale, lat.lengthscale)
    with torch.no_grad():
        a = lat(x, x) @ v
        b = twin(x, x) @ v
    assert rel_l2(b, dense64(x, x, v, "rbf")) <= 1e-5
    e = plx.mvm_error(a, b)
    assert all(math.isfinite(e[k]) for k in ("rel_err", "cos_err", "rel_l2"))
    assert e["cos_err"] > 0.9, e
    # the reference's formulas, evaluated directly on the same two outputs
    A, B = a.double().flatten(), b.double().flatten()
    S = A / (A / B).mean()
    ref_rel = ((B - S) ** 2).mean().sqrt() / ((B ** 2).mean().sqrt() + (S ** 2).mean().sqrt())
    ref_cos = (B * A).sum() / (B.norm() * A.norm())
    assert e["rel_err"] == pytest.approx(float(ref_rel), rel=1e-12)
    assert e["cos_err"] == pytest.approx(float(ref_cos), rel=1e-12)
    assert e["rel_l2"] == pytest.approx(float((A - B).norm() / B.norm()), rel=1e-12)


def test_large_call_sampled_rows():
    n, d = 200_000, 8
    x = points(n, d, 30)
    v = values(n, 1, 31)
    out = plx.exact_matmul(x, x, v, "rbf")
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(32))[:512].to(DEV)
    want = dense64(x[rows], x, v, "rbf")
    assert torch.isfinite(out).all()
    assert rel_l2(out[rows], want) <= 1e-5
