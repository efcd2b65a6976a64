"""The transposed and symmetrised fp32 lattice products (plx_blur_t, plx_apply_t, plx_blur_sym_work_floats, plx_blur_sym,
plx_apply_sym, plx_apply_affine_sym, plx_last_sym_kernels) on the host: the C ABI's declarations and exports, the refusals
that need no lattice, the dtype rule of the new Lattice methods, the two switches, and the routing of LatticeGP.khat_solve /
khat_in_lattice_rows and LatticeFilterGeneral.backward with the switches off (what they called before) and on."""
import ctypes
import re
import subprocess

import pytest
import torch

import simplex_gp_amd as plx
from simplex_gp_amd import _native
from simplex_gp_amd import lattice_kernel as lk
from simplex_gp_amd import solvers

SYMBOLS = {"plx_blur_t": 6, "plx_apply_t": 5, "plx_blur_sym_work_floats": 2, "plx_blur_sym": 6, "plx_apply_sym": 5,
           "plx_apply_affine_sym": 8, "plx_last_sym_kernels": 3}
PLX_ERR_INVALID = 1
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def test_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(_native.HEADER_PATH).read(), flags=re.S)
    declared = _native.declared_symbols()
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name, arity in SYMBOLS.items():
        assert name in declared and name in _native._SIGNATURES and name in _native.OPTIONAL_SYMBOLS, name
        assert hasattr(lib, name), name
        assert f" T {name}\n" in exported, name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(_native._SIGNATURES[name][1]), name
    # detected by symbol: version and ABI stay where they were
    assert lib.plx_version().decode() == "libplx 0.9.1 gfx950" and _native.ABI_VERSION == (0, 9)


def test_signatures():
    sig, vp, i64, i32 = _native._SIGNATURES, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert sig["plx_blur_t"] == sig["plx_blur"] == (i32, [vp, vp, vp, i32, ctypes.POINTER(i32), vp])
    assert sig["plx_apply_t"] == sig["plx_apply_sym"] == sig["plx_apply"] == (i32, [vp, vp, i32, vp, vp])
    assert sig["plx_blur_sym_work_floats"] == (i64, [vp, i32])
    assert sig["plx_blur_sym"] == (i32, [vp, vp, vp, i32, ctypes.POINTER(vp), vp])
    # (lat, src, vd, out, scale_shift, dot, work, stream): the argument list of plx_apply_affine_dot
    assert sig["plx_apply_affine_sym"] == sig["plx_apply_affine_dot"] == (i32, [vp, vp, i32, vp, vp, vp, vp, vp])
    assert sig["plx_last_sym_kernels"] == sig["plx_last_kernels"] == (i32, [vp, ctypes.c_char_p, i32])


def test_a_null_lattice_is_refused(lib):
    """PLX_ERR_INVALID before the lattice pointer is followed or anything is launched: the buffers are host addresses."""
    raw = (ctypes.c_float * 64)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    a, b, c, e = (ctypes.c_void_p(base + 16 * i) for i in range(4))
    flag, res = ctypes.c_int(0), ctypes.c_void_p(0)
    err = lib.plx_last_error
    assert lib.plx_blur_t(None, a, b, 2, ctypes.byref(flag), None) == PLX_ERR_INVALID and b"plx_blur_t" in err()
    assert lib.plx_apply_t(None, a, 2, b, None) == PLX_ERR_INVALID and b"plx_apply_t" in err()
    assert lib.plx_blur_sym(None, a, b, 2, ctypes.byref(res), None) == PLX_ERR_INVALID and b"plx_blur_sym" in err()
    assert lib.plx_apply_sym(None, a, 2, b, None) == PLX_ERR_INVALID and b"plx_apply_sym" in err()
    assert lib.plx_apply_affine_sym(None, a, 2, b, c, None, None, None) == PLX_ERR_INVALID and b"plx_apply_affine_sym" in err()
    assert lib.plx_apply_affine_sym(None, a, 2, b, c, e, e, None) == PLX_ERR_INVALID
    assert lib.plx_last_sym_kernels(None, ctypes.create_string_buffer(8), 8) == PLX_ERR_INVALID
    assert lib.plx_blur_sym_work_floats(None, 2) == -1
    assert res.value is None and flag.value == 0


def test_the_new_methods_take_float32_only():
    """A float64 tensor is refused by its dtype before anything else is looked at -- wherever it lives, so no lattice has
    to be built for it -- and the message names the float64 method."""
    lat = object.__new__(plx.Lattice)                  # no handle: the dtype rule comes before any use of it
    t64, t32 = torch.randn(6, 2, dtype=F64), torch.randn(6, 2)
    ss64, ss32 = torch.ones(2, dtype=F64), torch.ones(2)
    for call, name in ((lambda: lat.blur_t_f32(t64), "blur_t"), (lambda: lat.blur_sym_f32(t64), "blur_sym"),
                       (lambda: lat.apply_t_f32(t64), "apply_t"), (lambda: lat.apply_sym_f32(t64), "apply_sym"),
                       (lambda: lat.apply_t_f32(t32, out=t64), "apply_t"), (lambda: lat.apply_sym_f32(t32, out=t64), "apply_sym"),
                       (lambda: lat.apply_affine_sym_f32(t64, ss64), "apply_affine"),
                       (lambda: lat.apply_affine_sym_f32(t32, ss64), "apply_affine")):
        with pytest.raises(TypeError, match=r"float32 only.*float64 form is " + name):
            call()
    with pytest.raises(TypeError):
        lat.apply_sym_f32([[0.0]])
    # the float64 methods still refuse every float32 tensor
    for call in (lambda: lat.apply_t(t32), lambda: lat.apply_sym(t32), lambda: lat.blur_t(t32), lambda: lat.blur_sym(t32),
                 lambda: lat.apply_affine(t32, ss32, symmetric=True)):
        with pytest.raises(TypeError, match="float64 only"):
            call()
    assert callable(plx.Lattice.sym_kernels_f32)


def test_the_switches_exist_and_are_off():
    assert solvers.LatticeGP.symmetric_f32 is False and solvers.LatticeGP.symmetric_f64 is False
    assert plx.LatticeFilterGeneral.exact_adjoint_f32 is False and plx.LatticeFilterGeneral.exact_adjoint is False


# ---- routing ----------------------------------------------------------------------------------------------------------
class _StubLattice:
    """Records which product every closure of khat_solve / khat_in_lattice_rows / backward() reaches."""
    build_id = 1

    def __init__(self):
        self.calls, self.lattice_rows = [], []

    def set_lattice_row_order(self, on=True):
        self.lattice_rows.append(bool(on))

    def to_lattice_order(self, t):
        return t

    def from_lattice_order(self, t):
        return t

    def _affine(self, name, V, ss, want_dot):
        self.calls.append((name, want_dot))
        out = 2.0 * V
        if want_dot == "partial":
            return out, torch.zeros(4), 1
        return (out, (V * out).sum(0)) if want_dot else out

    def apply_affine(self, V, ss, out=None, want_dot=False):
        return self._affine("apply_affine", V, ss, want_dot)

    def apply_affine_sym_f32(self, V, ss, out=None, want_dot=False):
        return self._affine("apply_affine_sym_f32", V, ss, want_dot)

    def apply(self, V):
        self.calls.append(("apply", False))
        return 2.0 * V

    def apply_sym_f32(self, V):
        self.calls.append(("apply_sym_f32", False))
        return 2.0 * V

    def apply_t_f32(self, g):
        self.calls.append(("apply_t_f32", False))
        return 3.0 * g


class _DevicePositions:
    """What khat_solve asks of `x` before it reaches the lattice: a device float32 tensor it divides by the lengthscale."""
    is_cuda, dtype = True, F32

    def __init__(self, t):
        self.t = t

    def div(self, ls):
        return self.t / ls


def _drive(monkeypatch, symmetric):
    """khat_solve (native branch, caller-order branch) and khat_in_lattice_rows on a stub lattice, with batched_cg and the
    refinement replaced by drivers that call every closure they are handed once."""
    stub = _StubLattice()

    class _Cache:
        def get(self, ref, coeffs):
            return stub

    def fake_cg(matmul, B, matmul_dot=None, native_precond=False, **kw):
        matmul(B)
        if matmul_dot is not None:
            matmul_dot(B)
            matmul_dot.partial(B)
        return torch.zeros_like(B), {"iterations": 1, "residual": torch.zeros(B.shape[1])}

    def fake_refine(matmul, B, X, info, matmul_dot, native_pre, cg_args):
        matmul(B)
        return X, info

    monkeypatch.setattr(lk, "lattice_cache", lambda: _Cache())
    monkeypatch.setattr(solvers, "batched_cg", fake_cg)
    monkeypatch.setattr(solvers, "_refine_solution", fake_refine)
    model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=2))
    model.symmetric_f32 = symmetric
    x = _DevicePositions(torch.randn(8, 2))
    rhs = torch.randn(8, 3)
    model.khat_solve(x, rhs, tol=1e-6)
    native = list(stub.calls)
    stub.calls.clear()
    model.khat_solve(x, rhs, tol=1e-6, precond=object())          # not the native preconditioner: the caller's row order
    caller = list(stub.calls)
    stub.calls.clear()
    with model.khat_in_lattice_rows(x) as (mm, to_rows, from_rows):
        mm(rhs)
    rows = list(stub.calls)
    assert stub.lattice_rows[-1] is False                          # every path leaves the caller's row order behind
    return native, caller, rows


def test_khat_routing_with_the_switch_off_is_what_it_was(monkeypatch):
    native, caller, rows = _drive(monkeypatch, False)
    # the iteration's MVM, its fused dot, the partial form of it, the refinement's MVM: all plx_apply_affine[_dot]
    assert native == [("apply_affine", False), ("apply_affine", True), ("apply_affine", "partial"), ("apply_affine", False)]
    assert caller == [("apply", False)]
    assert rows == [("apply_affine", False)]


def test_khat_routing_with_the_switch_on(monkeypatch):
    native, caller, rows = _drive(monkeypatch, True)
    name = "apply_affine_sym_f32"
    assert native == [(name, False), (name, True), (name, "partial"), (name, False)]
    assert caller == [("apply_sym_f32", False)]
    assert rows == [(name, False)]


class _Ctx:
    pass


class _CudaLike(torch.Tensor):
    """A host tensor that says it is on the device: enough for backward()'s routing predicate."""
    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("device_like", [False, True])
def test_backward_routing(monkeypatch, switch, device_like):
    """grad_source of a source-only backward: the forward-tap filter of g (K g) unless the switch is on AND the tensors are
    device float32 2-D with `method` None; then apply_t_f32 on the forward-tap lattice and no filter at all."""
    stub = _StubLattice()
    filtered = []

    def fake_filter(src, ref, coeffs):
        filtered.append(coeffs)
        return 2.0 * src

    monkeypatch.setattr(lk._cache, "get", lambda positions, coeffs: stub)
    monkeypatch.setattr(lk, "cached_filter", fake_filter)
    monkeypatch.setattr(lk.LatticeFilterGeneral, "exact_adjoint_f32", switch)
    assert lk.LatticeFilterGeneral.method is None
    mk = (lambda t: t.as_subclass(_CudaLike)) if device_like else (lambda t: t)
    ctx = _Ctx()
    ctx.needs_input_grad = (True, False, False)
    ctx.saved_tensors = (mk(torch.ones(5, 2)), mk(torch.ones(5, 3)))
    ctx.coeffs, ctx.deriv_coeffs = "forward taps", "derivative taps"
    g = mk(torch.ones(5, 2))
    grad_source, grad_reference, _ = lk.LatticeFilterGeneral.backward(ctx, g)
    assert grad_reference is None
    if switch and device_like:
        assert stub.calls == [("apply_t_f32", False)] and filtered == []
        assert torch.equal(torch.as_tensor(grad_source).as_subclass(torch.Tensor), 3.0 * torch.ones(5, 2))
    else:
        assert stub.calls == [] and filtered == ["forward taps"]
        assert torch.equal(torch.as_tensor(grad_source).as_subclass(torch.Tensor), 2.0 * torch.ones(5, 2))
    # float64 tensors never take the fp32 route
    stub.calls.clear(); filtered.clear()
    ctx.saved_tensors = (mk(torch.ones(5, 2, dtype=F64)), mk(torch.ones(5, 3, dtype=F64)))
    lk.LatticeFilterGeneral.backward(ctx, mk(torch.ones(5, 2, dtype=F64)))
    assert stub.calls == [] and filtered == ["forward taps"]
