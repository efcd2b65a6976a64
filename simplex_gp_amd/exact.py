"""The exact kernel MVM (plx_exact_mvm / plx_exact_grad and their _f64 twins, HIP) behind the same operator surface as
the lattice.

    exact_matmul(x1, x2, v, profile)   K(x1, x2) @ v, autograd for v, x1 and x2; nothing N x N is stored
    ExactLazyKernel                    K(x1, x2) known through its action (the protocol of SquareLazyLattice)
    ExactKernel, RBFExact, MaternExact the GPyTorch-facing kernels (ARD lengthscale, as LatticeAccelerated)
    exact_twin(lattice_kernel)         the ExactKernel a lattice kernel approximates: same profile, same lengthscale
    mvm_error(lattice_out, exact_out)  how far a lattice MVM is from the exact one

The profiles are the project's own (stencil.py): "rbf" is exp(-d2), "matern12/32/52" the Matern-nu profiles of
r = sqrt(d2).  This is what the lattice stands in for, so the exact operator measures the lattice's approximation error
and gives the like-for-like "lattice vs exact on the same GPU" speed figure.  float32 tensors run the fp32 kernels,
float64 tensors the double ones (plx_exact_f64.hip: every operation in double, so torch.autograd.gradcheck applies); the
three tensors of a call share one dtype.  There is no CPU path.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _native as nv
from .gp_compat import Kernel, LazyTensor

F64_SYMBOLS = ("plx_exact_work_bytes_f64", "plx_exact_splits_f64", "plx_exact_mvm_f64", "plx_exact_grad_f64")
PROFILES = {"rbf": nv.PROFILE_RBF, "matern12": nv.PROFILE_MATERN12, "matern32": nv.PROFILE_MATERN32,
            "matern52": nv.PROFILE_MATERN52}
_MATERN_PROFILE = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}


def _profile_code(profile):
    if profile not in PROFILES:
        raise ValueError(f"unknown profile {profile!r}: one of {sorted(PROFILES)}")
    return PROFILES[profile]


def _check(x1, x2, v):
    floats = {t.dtype for t in (x1, x2, v) if isinstance(t, torch.Tensor)}
    if floats == {torch.float32, torch.float64}:              # wherever the tensors live: as the lattice's filter
        raise TypeError(f"x1, x2 and v must share one dtype (got {x1.dtype}, {x2.dtype}, {v.dtype})")
    for name, t in (("x1", x1), ("x2", x2), ("v", v)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"simplex_gp_amd has no CPU path: {name} must live on an MI355X (cuda) device")
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"float32 or float64 only (got {name} {t.dtype})")
    if x1.dtype == torch.float64 and not nv.has_symbols(*F64_SYMBOLS):
        raise TypeError("float64 tensors need a libplx.so that exports " + ", ".join(F64_SYMBOLS) + ": rebuild it")
    if x1.dim() != 2 or x2.dim() != 2 or v.dim() != 2:
        raise ValueError(f"x1 [n1, d], x2 [n2, d] and v [n2, t] are matrices (got {tuple(x1.shape)}, {tuple(x2.shape)}, "
                         f"{tuple(v.shape)})")
    if x1.shape[1] != x2.shape[1]:
        raise ValueError(f"x1 and x2 differ in d ({x1.shape[1]} vs {x2.shape[1]})")
    if v.shape[0] != x2.shape[0]:
        raise ValueError(f"v has {v.shape[0]} rows, x2 has {x2.shape[0]}")
    if x1.device != x2.device or v.device != x1.device:
        raise ValueError(f"x1 ({x1.device}), x2 ({x2.device}) and v ({v.device}) must live on the same device")


def _call(fn, x1, x2, a, b, t, out):
    """One plx_exact_mvm (b is None) or plx_exact_grad on the current stream, the workspace from torch's allocator; the
    _f64 entry points and their workspace bound where the tensors are float64."""
    L = nv.lib()
    n1, d = x1.shape
    n2 = x2.shape[0]
    f64 = x1.dtype == torch.float64
    work_bytes, mvm, grad = ((L.plx_exact_work_bytes_f64, L.plx_exact_mvm_f64, L.plx_exact_grad_f64) if f64 else
                             (L.plx_exact_work_bytes, L.plx_exact_mvm, L.plx_exact_grad))
    who = ("plx_exact_mvm" if b is None else "plx_exact_grad") + ("_f64" if f64 else "")
    nbytes = work_bytes(n1, n2, d, t)
    if nbytes < 0:
        raise ValueError(f"sizes outside the exact kernel's limits: n1 = {n1}, n2 = {n2}, d = {d}, t = {t}")
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x1.device)
    ptr = lambda z: ctypes.c_void_p(z.data_ptr())            # noqa: E731
    with torch.cuda.device(x1.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(x1.device).cuda_stream)
        if b is None:
            rc = mvm(ptr(x1), n1, ptr(x2), n2, d, fn, ptr(a), t, ptr(out), ptr(work), work.numel(), stream)
        else:
            rc = grad(ptr(x1), n1, ptr(x2), n2, d, fn, ptr(a), ptr(b), t, ptr(out), ptr(work), work.numel(), stream)
        nv.check(rc, who)
    return out


def _mvm(x1, x2, v, code):
    out = torch.empty((x1.shape[0], v.shape[1]), dtype=x1.dtype, device=x1.device)
    return _call(code, x1.contiguous(), x2.contiguous(), v.contiguous(), None, v.shape[1], out)


def _grad(x1, x2, g, v, code):
    """sum_j 2 k'(d2_ij) (x1_i - x2_j) (g_i . v_j): the position gradient of sum_i g_i . (K(x1, x2) v)_i for x1."""
    out = torch.empty_like(x1, memory_format=torch.contiguous_format)
    return _call(code, x1.contiguous(), x2.contiguous(), g.contiguous(), v.contiguous(), v.shape[1], out)


class ExactMatmul(Function):
    """K(x1, x2) @ v with k the profile `code`; gradients: v through the forward kernel with the roles swapped,
    x1 and x2 through plx_exact_grad (x2's with the roles swapped).  x1 is x2: autograd sums the two position gradients."""

    @staticmethod
    def forward(ctx, x1, x2, v, code):
        ctx.code = code
        ctx.save_for_backward(x1, x2, v)
        return _mvm(x1, x2, v, code)

    @staticmethod
    def backward(ctx, g):
        x1, x2, v = ctx.saved_tensors
        g = g.contiguous()
        grad_x1 = grad_x2 = grad_v = None
        with torch.no_grad():
            if ctx.needs_input_grad[2]:
                grad_v = _mvm(x2, x1, g, ctx.code)
            if ctx.needs_input_grad[0]:
                grad_x1 = _grad(x1, x2, g, v, ctx.code)
            if ctx.needs_input_grad[1]:
                grad_x2 = _grad(x2, x1, v, g, ctx.code)
        return grad_x1, grad_x2, grad_v, None


def exact_matmul(x1, x2, v, profile="rbf"):
    """K(x1, x2) @ v, K[i, j] = k(|x1_i - x2_j|^2) with k one of PROFILES, on the GPU (positions already divided by the
    lengthscale).  x1, x2 and v share one dtype, float32 or float64, and the product is evaluated and returned in it.
    v: [n2, t] or [n2].  Differentiable in x1, x2 and v."""
    code = _profile_code(profile)
    vec = isinstance(v, torch.Tensor) and v.dim() == 1
    v2 = v.unsqueeze(-1) if vec else v
    _check(x1, x2, v2)
    out = ExactMatmul.apply(x1, x2, v2, code)
    return out.squeeze(-1) if vec else out


class ExactLazyKernel(LazyTensor):
    """K(x1, x2), known through its action only, evaluated exactly on the fly: the protocol of SquareLazyLattice /
    RectangularLazyLattice (_matmul, _size, _transpose_nonbatch with the roles swapped, diag = ones, k(0) = 1)."""

    def __init__(self, x1, x2, profile="rbf"):
        super().__init__(x1, x2, profile=profile)
        _profile_code(profile)
        self.x1, self.x2, self.profile = x1, x2, profile

    def _size(self):
        return torch.Size((self.x1.shape[-2], self.x2.shape[-2]))

    def _matmul(self, V):
        return exact_matmul(self.x1, self.x2, V, self.profile)

    def _transpose_nonbatch(self):
        return type(self)(self.x2, self.x1, self.profile)

    def diag(self):
        if self.x1 is not self.x2:
            raise RuntimeError("diag of a rectangular kernel matrix")
        return self.x1.new_ones(self.x1.shape[:-1])


class ExactKernel(Kernel):
    """A stationary kernel with one of the project's profiles, evaluated exactly: the inputs are divided by the (ARD)
    lengthscale as LatticeAccelerated.forward does, and the product runs through plx_exact_mvm."""

    has_lengthscale = True

    def __init__(self, profile="rbf", *args, **kwargs):
        _profile_code(profile)
        super().__init__(*args, **kwargs)
        self.profile = profile

    def forward(self, x1, x2, diag=False, **params):
        if diag:
            return x1.new_ones(x1.shape[:-1])
        scaled1 = x1.div(self.lengthscale)
        if x1 is x2:
            return ExactLazyKernel(scaled1, scaled1, self.profile)
        return ExactLazyKernel(scaled1, x2.div(self.lengthscale), self.profile)


def RBFExact(*args, **kwargs):
    """exp(-|x1 - x2|^2 / l^2): the exact twin of RBFLattice (the lattice's RBF, not GPyTorch's exp(-d2 / 2))."""
    return ExactKernel("rbf", *args, **kwargs)


def MaternExact(*args, nu=1.5, **kwargs):
    """The Matern-nu profile of r = |x1 - x2| / l, nu in {0.5, 1.5, 2.5}: the exact twin of MaternLattice."""
    if nu not in _MATERN_PROFILE:
        raise ValueError(f"Matern nu={nu}: one of {sorted(_MATERN_PROFILE)}")
    return ExactKernel(_MATERN_PROFILE[nu], *args, **kwargs)


def exact_twin(lattice_kernel):
    """The ExactKernel with the profile and the lengthscale values of `lattice_kernel` (made by RBFLattice,
    BilateralKernel or MaternLattice), on the same device and in the same dtype (the twin of a double model's kernel is a
    double kernel).  A LatticeAccelerated built from any other callable has no known profile: ValueError."""
    profile = getattr(lattice_kernel, "profile", None)
    if profile not in PROFILES:
        raise ValueError("exact_twin: the kernel's profile is not one of the project's (build it with RBFLattice, "
                         "BilateralKernel or MaternLattice)")
    ls = lattice_kernel.lengthscale.detach()
    twin = ExactKernel(profile, ard_num_dims=getattr(lattice_kernel, "ard_num_dims", None))
    twin = twin.to(device=ls.device, dtype=ls.dtype)
    twin.lengthscale = ls
    return twin


def mvm_error(lattice_out, exact_out):
    """How far a lattice MVM is from the exact one: {"rel_err", "cos_err", "rel_l2"} (floats).

    rel_err: the reference's experiment (experiments/mvm_err.py:11-12, :94): the lattice output a is first rescaled by
        the mean of the element-wise ratio a / b, then rel_err = rms(b - a') / (rms(b) + rms(a'));
    cos_err: the cosine of the angle between the two flattened outputs, (a . b) / (|a| |b|) (:15-16) -- 1 is a perfect
        direction;
    rel_l2: |a - b|_2 / |b|_2, without any rescale.
    Everything is evaluated in fp64.  Beware when comparing with the reference's published numbers: its RBF pairing
    compared the lattice's exp(-d2) with GPyTorch's exact exp(-d2 / 2) (tools/mvm_err.py --gpytorch-rbf reproduces it);
    the kernels here pair like with like.
    """
    a = lattice_out.detach().double().reshape(-1)
    b = exact_out.detach().double().reshape(-1)
    scaled = a / (a / b).mean()
    rms = lambda z: z.square().mean().sqrt()                 # noqa: E731
    rel_err = rms(b - scaled) / (rms(b) + rms(scaled))
    cos_err = (a * b).sum() / (a.norm() * b.norm())
    rel_l2 = (a - b).norm() / b.norm()
    return {"rel_err": float(rel_err), "cos_err": float(cos_err), "rel_l2": float(rel_l2)}
