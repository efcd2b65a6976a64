"""Operator surface: the autograd op and the GPyTorch-facing kernel classes.

Mirrors gpytorch_lattice_kernel/bilateral_kernel.py (same names, constructor
arguments, shapes and error behaviour):
    LatticeFilterGeneral      py:59-124    forward = one filter, backward = one wider filter
    SquareLazyLattice         py:127-140   RectangularLazyLattice   py:142-160
    LatticeAccelerated        py:183-200
    RBFLattice / BilateralKernel / MaternLattice   py:247-254

What differs on purpose: the native call goes to libplx (HIP, gfx950) through
the C ABI, and the lattice built for a given (positions, taps) pair is kept and
reused by every later MVM on the same positions (all CG iterations call
_matmul with the same x / lengthscale tensor), instead of being rebuilt inside
every filter call (permutohedral.h:272).
"""
from collections import OrderedDict

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .gp_compat import Kernel, LazyTensor
from .lattice import Lattice, _taps_array
from .stencil import DiscretizedKernelFN, Matern, rbf


# ---- warm start of the point order across re-scaled rebuilds -----------------------------------------------------------
# A training step divides the SAME data tensor by a lengthscale that moved a little (py:198-200) and builds a new lattice on
# the result.  The build's first stage orders the points along a space-filling curve -- a locality device only, nothing in
# the structure depends on it -- and that order survives a re-scaling (measured, N = 1e6, d = 8, tools/ab_reuse_order_r6.py:
# the order of l = 0.69 kept for l x 0.8 ... x 2: build -0.13 ... -0.17 ms of 0.5 ... 2.1, the MVMs as fast or faster).
# So a scaled tensor remembers which data tensor it came from (position_hint), and a cache miss whose hint matches an
# entry's rebuilds THAT entry's lattice in place with its point order kept (Lattice.build(reuse_order=True)).
MAX_ORDER_AGE = 8          # rebuilds before the order is computed afresh (Adam at lr 0.1 moves a lengthscale < 2.2x in 8 steps)


def position_hint(scaled, source, scale_of=None):
    """Mark `scaled` as positions derived from the data tensor `source` by a re-scaling (returns `scaled`).
    scale_of: the tensor the scale is a deterministic function of (the kernel's raw lengthscale PARAMETER; the lengthscale
    itself is a fresh softplus output on every access).  Two hints with the same source whose scale_of is the same tensor
    holding the same VALUES mark bit-identical positions: the cache then serves the lattice it has instead of rebuilding it
    (an evaluation followed by the next training step: the same hyper-parameters twice).  The values are compared on the
    device (d floats and one read-back, only when identity and version counter already agree): the version counter alone
    cannot vouch for them -- torch.optim.Adam(fused=True) writes parameters without moving it (measured on this image).
    The hint: ((weak reference, version, shape) per source tensor, scale key); stack_hint() joins the hints of stacked parts."""
    import weakref
    try:
        scale_key = None if scale_of is None else (weakref.ref(scale_of), scale_of._version)
        scaled._plx_positions_of = (((weakref.ref(source), source._version, tuple(source.shape)),), scale_key)
    except (AttributeError, TypeError):
        pass
    return scaled


def stack_hint(stacked, parts):
    """`stacked` is the concatenation of `parts` (the rectangular operator's [xout; xin], py:150-156): if every part says
    which data tensor it was scaled from, and by the same scale, the stack says so for all of them -- the stacked lattice of
    the SAME two data tensors under a moved lengthscale (the validation split, epoch after epoch) is then rebuilt in place
    with its point order kept instead of piling up in the cache as a new lattice per epoch."""
    hints = [getattr(p, "_plx_positions_of", None) for p in parts]
    if any(h is None for h in hints):
        return stacked
    scale = hints[0][1]
    for h in hints[1:]:
        if (h[1] is None) != (scale is None) or (scale is not None and (h[1][0]() is not scale[0]() or h[1][1] != scale[1])):
            return stacked
    try:
        stacked._plx_positions_of = (tuple(src for h in hints for src in h[0]), scale)
    except (AttributeError, TypeError):
        pass
    return stacked


def carry_hint(dst, src):
    """dst is src under another tensor object (detach / contiguous): keep the hint."""
    h = getattr(src, "_plx_positions_of", None)
    if h is not None and dst is not src:
        try:
            dst._plx_positions_of = h
        except (AttributeError, TypeError):
            pass
    return dst


def _same_hint(a, b):
    """Both hints name the same live data tensors, in the same states, and none has been written since."""
    if a is None or b is None or len(a[0]) != len(b[0]):
        return False
    for (ra, va, sa), (rb, vb, sb) in zip(a[0], b[0]):
        src = ra()
        if src is None or src is not rb() or va != vb or sa != sb or src._version != va:
            return False
    return True


def _scale_tensor(hint):
    """The live parameter a hint's scale comes from, or None."""
    k = hint[1] if hint is not None else None
    return None if k is None else k[0]()


def _same_scale(a, b, snapshot):
    """Both hints name the same live scale parameter, its version counter has not moved since either was made, and it
    still holds the values `snapshot` (taken when the lattice was built) -- the last by comparison on the device."""
    ka, kb = a[1], b[1]
    if ka is None or kb is None or snapshot is None:
        return False
    p = ka[0]()
    if p is None or p is not kb[0]() or not (ka[1] == kb[1] == p._version) or snapshot.shape != p.shape:
        return False
    return bool(torch.equal(snapshot, p.detach()))


def _snapshot_scale(hint):
    p = _scale_tensor(hint)
    return None if p is None else p.detach().clone()


def _build_positions(ref):
    """What Lattice.build gets for the cached position tensor `ref`: float64 positions rounded to float32 (the float64
    product runs on the fp32 build's lattice), everything else as it is (build() does the checking)."""
    return ref.to(torch.float32) if ref.dtype == torch.float64 else ref


class _LatticeCache:
    """Small LRU of built lattices keyed on the position tensor and the taps.

    An entry holds a reference to its position tensor, so the allocator cannot
    hand the same address to different data while the entry lives; together
    with tensor._version that makes (data_ptr, _version, shape, taps) a sound key
    for every write torch knows about.  Writes that bypass the version counter
    (`x.data.copy_()`, a custom kernel or a DLPack alias writing into the same
    storage) are NOT seen: call lattice_cache().clear() after such a write.

    float64 positions are keyed (and kept alive) as the tensor they are and built on their rounding to float32
    (_build_positions): the lattice of a float64 tensor serves float64 and float32 right-hand sides alike; the same
    positions held once in each dtype are two tensors, hence two entries.
    """

    def __init__(self, capacity=4):
        self.capacity = capacity
        self._entries = OrderedDict()
        self.hits = 0
        self.misses = 0
        self.warm_rebuilds = 0             # misses served by rebuilding an entry of the same data in place (point order kept)
        self.same_positions = 0            # new position tensors recognised as the positions of an entry (same data, same scale state)

    @staticmethod
    def _key(ref, taps):
        return (ref.device.index, ref.data_ptr(), ref._version, tuple(ref.shape), taps.tobytes())

    def get(self, ref, coeffs):
        taps = _taps_array(coeffs)
        key = self._key(ref, taps)
        hit = self._entries.get(key)
        if hit is not None:
            self._entries.move_to_end(key)
            self.hits += 1
            return hit[0]
        self.misses += 1
        # the same data under a lengthscale that moved: rebuild that entry's lattice in place, point order kept
        hint = getattr(ref, "_plx_positions_of", None)
        if hint is not None:
            for k2, (lat2, ref2, snap2) in self._entries.items():
                hint2 = getattr(ref2, "_plx_positions_of", None)
                if (k2[0], k2[3], k2[4]) == (key[0], key[3], key[4]) and _same_hint(hint, hint2):
                    del self._entries[k2]
                    if _same_scale(hint, hint2, snap2):
                        # the same data divided by the same lengthscale, as a new tensor: the positions this lattice was
                        # built on.  The entry moves under the new tensor (the one the caller will come back with).
                        self._entries[key] = (lat2, ref, snap2)
                        self.misses -= 1
                        self.hits += 1
                        self.same_positions += 1
                        return lat2
                    keep = 0 <= lat2.order_age < MAX_ORDER_AGE      # (an order that old is computed afresh, in place all the same)
                    lat2.build(_build_positions(ref), taps, reuse_order=keep)
                    self._entries[key] = (lat2, ref, _snapshot_scale(hint))
                    self.warm_rebuilds += 1 if keep else 0
                    return lat2
        if len(self._entries) >= self.capacity:
            _, (old, _, _) = self._entries.popitem(last=False)
            lat = old                      # recycle the device buffers of the evicted lattice
        else:
            lat = Lattice(ref.device)
        lat.build(_build_positions(ref), taps)
        self._entries[key] = (lat, ref, _snapshot_scale(hint))
        return lat

    def clear(self):
        for lat, _, _ in self._entries.values():
            lat.close()
        self._entries.clear()


_cache = _LatticeCache()


def lattice_cache():
    return _cache


def cached_filter(src, ref, coeffs):
    """filter(src, ref, coeffs) with the lattice for (ref, coeffs) reused when
    the same position tensor comes back (the CG loop, the backward pass).  Both float64: the product runs in double on
    the lattice of the positions rounded to float32 (Lattice.apply)."""
    if isinstance(src, torch.Tensor) and isinstance(ref, torch.Tensor) and src.dtype != ref.dtype:
        raise TypeError(f"src and ref must both be float32 or both float64 (got src {src.dtype}, ref {ref.dtype})")
    if not (isinstance(src, torch.Tensor) and src.is_cuda):
        raise ValueError("simplex_gp_amd has no CPU path: tensors must live on an MI355X (cuda) device")
    if src.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"float32 or float64 only (got src {src.dtype}, ref {ref.dtype})")
    if not ref.is_cuda or ref.device != src.device:
        # checked before the cache is touched: a bad call must not evict a good lattice
        raise ValueError(f"src ({src.device}) and ref ({ref.device}) must live on the same MI355X (cuda) device")
    lat = _cache.get(ref if ref.is_contiguous() else carry_hint(ref.contiguous(), ref), coeffs)
    return lat.apply(src)


class LatticeFilterGeneral(Function):
    """out = K(reference) @ source, K the lattice approximation of the kernel
    whose taps come from `kernel_fn` (a DiscretizedKernelFN).

    `method` is the native filter used, as in the reference (py:60, py:94-95):
    None selects the HIP path; tests may install another callable with the
    reference's filter(src, ref, coeffs) signature.
    """

    method = None
    fused_backward = True      # False: position gradient through plx_backward_stack / filter / plx_backward_contract
    # float64: True sends the position gradient of a CUDA 2-D double right-hand side through plx_apply_backward_f64 (stack
    # formed inside the splat, contraction inside the slice; Lattice.backward_f64_ok shapes); False keeps the torch stack
    # and contraction around the native fp64 product.  The two routes agree to rounding, so the
    # switch changes time and memory only.  Off until the native route has been measured no slower than the torch route
    # at the three shapes of tools/backward_f64_time.py (profiles/backward_f64_measured.md).
    fused_backward_f64 = False
    # float64: True returns the EXACT adjoint for the gradient with respect to `source`: K^T g on the forward-tap lattice
    # (Lattice.apply_t), in every branch of backward() that returns one -- K is not symmetric, so neither K g (py:110-111)
    # nor the derivative-tap filter of g (py:123) is the adjoint of the forward product, and torch.autograd.gradcheck with
    # respect to `source` fails without the switch.  Applies where `method` is None and the tensors are CUDA float64 2-D.
    # The POSITION gradient is unchanged: it keeps the reference's symmetric treatment (py:113-122).  Off by default: the
    # reference's gradients are what every existing caller and test sees.
    exact_adjoint = False
    # float32: the same switch for the default precision: grad_source = Lattice.apply_t_f32(g) (plx_apply_t) on the
    # forward-tap lattice, in every branch of backward() that returns one, where `method` is None and the tensors are CUDA
    # float32 2-D.  The position gradient is unchanged.  Off by default.
    exact_adjoint_f32 = False

    @staticmethod
    def _filter():
        return LatticeFilterGeneral.method if LatticeFilterGeneral.method is not None else cached_filter

    @staticmethod
    def forward(ctx, source, reference, kernel_fn):
        assert source.shape[0] == reference.shape[0], \
            "Incompatible shapes {}, and {}".format(source.shape, reference.shape)
        coeffs = kernel_fn.get_coeffs()
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(source, reference)
            ctx.coeffs = coeffs
            ctx.deriv_coeffs = kernel_fn.get_deriv_coeffs()
        return LatticeFilterGeneral._filter()(source, carry_hint(reference.contiguous(), reference), coeffs)

    @staticmethod
    def backward(ctx, grad_output):
        filt = LatticeFilterGeneral._filter()
        grad_source = grad_reference = None
        with torch.no_grad():
            src, ref = ctx.saved_tensors
            g = grad_output
            L = src.shape[-1]
            d = ref.shape[-1]
            exact = (LatticeFilterGeneral.exact_adjoint and LatticeFilterGeneral.method is None and ctx.needs_input_grad[0]
                     and g.is_cuda and g.dim() == 2 and g.dtype == src.dtype == ref.dtype == torch.float64)
            exact32 = (LatticeFilterGeneral.exact_adjoint_f32 and LatticeFilterGeneral.method is None
                       and ctx.needs_input_grad[0] and g.is_cuda and g.dim() == 2
                       and g.dtype == src.dtype == ref.dtype == torch.float32)
            want_src = ctx.needs_input_grad[0] and not (exact or exact32)      # (exact: grad_source is formed once, at the end)
            if want_src and not ctx.needs_input_grad[1]:
                # K is treated as symmetric (py:110-111)
                grad_source = filt(g.contiguous(), ref.contiguous(), ctx.coeffs)
            # float32: the fused and the three-call position gradients are fp32 kernels.  In double the gradient is one
            # native call too where fused_backward_f64 is on (plx_apply_backward_f64); otherwise the stack and the
            # contraction below are torch in float64 around the native fp64 product on the derivative-tap lattice.
            native = LatticeFilterGeneral.method is None and g.is_cuda and g.dim() == 2 and g.dtype == torch.float32
            native64 = (LatticeFilterGeneral.fused_backward_f64 and LatticeFilterGeneral.method is None and g.is_cuda
                        and g.dim() == 2 and g.dtype == src.dtype == ref.dtype == torch.float64
                        and Lattice.backward_f64_ok(L, d))
            lat64 = None
            if ctx.needs_input_grad[1] and native64:
                rc_ = ref if ref.is_contiguous() else carry_hint(ref.contiguous(), ref)
                lat64 = _cache.get(rc_, ctx.deriv_coeffs)
                if not lat64.accepts_rows():         # a sharded, merged or replayed build: the torch route serves it
                    lat64 = None
            if ctx.needs_input_grad[1] and native and LatticeFilterGeneral.fused_backward and Lattice.backward_fusable(L, d):
                # the whole of py:113-123 in one native call: the stacked matrix is never stored (plx_apply_backward)
                rc_ = ref if ref.is_contiguous() else carry_hint(ref.contiguous(), ref)
                lat = _cache.get(rc_, ctx.deriv_coeffs)
                grad_reference, grad_source = lat.apply_backward(g, src, rc_, want_grad_src=want_src)
            elif ctx.needs_input_grad[1] and lat64 is not None:
                # the same in double: stack inside the splat, contraction inside the slice (plx_apply_backward_f64)
                grad_reference, grad_source = lat64.apply_backward(g, src, rc_, want_grad_src=want_src)
            elif ctx.needs_input_grad[1] and native:
                # same computation, the stack and the contraction each as one native pass (plx_backward_*)
                import ctypes
                from . import _native as nv
                n = src.shape[0]
                gc, sc, rc_ = g.contiguous(), src.contiguous(), ref.contiguous()
                stacked = torch.empty((n, 2 * L * (1 + d)), dtype=torch.float32, device=g.device)
                ptr = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
                stream = ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
                with torch.cuda.device(g.device):
                    nv.check(nv.lib().plx_backward_stack(ptr(gc), ptr(sc), ptr(rc_), n, L, d, ptr(stacked), stream),
                             "plx_backward_stack")
                filtered = filt(stacked, rc_, ctx.deriv_coeffs)
                del stacked
                grad_reference = torch.empty_like(rc_)
                with torch.cuda.device(g.device):
                    nv.check(nv.lib().plx_backward_contract(ptr(gc), ptr(sc), ptr(rc_), ptr(filtered), n, L, d,
                                                            ptr(grad_reference), stream), "plx_backward_contract")
                if want_src:
                    grad_source = filtered[:, :L].contiguous()   # filtered with the derivative taps (py:123)
            elif ctx.needs_input_grad[1]:
                # one filter with the derivative taps over [g, g (x) x, src, src (x) x]   (py:113-119)
                gx = (g[..., None] * ref[..., None, :])          # n x L x d
                sx = (src[..., None] * ref[..., None, :])
                stacked = torch.cat([g, gx.reshape(gx.shape[:-2] + (L * d,)),
                                     src, sx.reshape(sx.shape[:-2] + (L * d,))], dim=-1)
                filtered = filt(stacked.contiguous(), ref.contiguous(), ctx.deriv_coeffs)
                wg, wgx, ws, wsx = torch.split(filtered, [L, L * d, L, L * d], dim=-1)
                wgx = wgx.reshape(-1, L, d)
                wsx = wsx.reshape(-1, L, d)
                # py:122
                grad_reference = -2 * (sx * wg[..., None] - src[..., None] * wgx
                                       + gx * ws[..., None] - g[..., None] * wsx).sum(-2)
                if want_src:
                    grad_source = wg       # filtered with the derivative taps, as the reference does (py:123)
            if exact:
                # the adjoint of the forward product: K^T g with the forward taps (plx_apply_t_f64)
                rc_ = ref if ref.is_contiguous() else carry_hint(ref.contiguous(), ref)
                grad_source = _cache.get(rc_, ctx.coeffs).apply_t(g.contiguous())
            elif exact32:
                # ... and in float32 (plx_apply_t)
                rc_ = ref if ref.is_contiguous() else carry_hint(ref.contiguous(), ref)
                grad_source = _cache.get(rc_, ctx.coeffs).apply_t_f32(g.contiguous())
        return grad_source, grad_reference, None


class LatticeRowsProduct(Function):
    """out = K[out rows, src rows] @ source on the lattice of `positions` (the stacked points of a rectangular operator):
    only the rows that carry a right-hand side are splatted, only the wanted rows are sliced (plx_apply_rows).  The
    gradient with respect to `source` is the transposed product on the same lattice, ranges swapped (K is treated as
    symmetric, py:110-111).

    Position gradient: only with the discretised kernel as the trailing argument (RectangularLazyLattice passes it where
    native_rows_grad_f64 sends a float64 product here, or native_rows_grad a float32 one); without it there is none and RectangularLazyLattice keeps the
    padded path for that.  It is py:113-123 split by sides -- the incoming gradient lives on the out rows only, the
    right-hand side on the source rows only -- into two one-sided calls on the derivative-tap lattice of the stacked
    positions (Lattice.apply_backward_rows; for float32 positions Lattice.apply_backward_rows_f32,
    section 22), added into one zero [n, d] tensor; grad_source is then
    the derivative-tap filter of the incoming gradient, as LatticeFilterGeneral.backward returns it (py:123)."""

    @staticmethod
    def forward(ctx, source, positions, coeffs, lat, src_begin, out_begin, out_count, kernel_fn=None):
        ctx.coeffs = coeffs
        ctx.ranges = (int(src_begin), int(source.shape[0]), int(out_begin), int(out_count))
        ctx.deriv_coeffs = None
        if kernel_fn is not None and ctx.needs_input_grad[1]:
            ctx.deriv_coeffs = kernel_fn.get_deriv_coeffs()
            ctx.save_for_backward(source, positions)
        else:
            ctx.positions = positions
        return lat.apply_rows(source, src_begin, out_begin, out_count)

    @staticmethod
    def backward(ctx, grad_output):
        grad_source = grad_positions = None
        sb, sc, ob, oc = ctx.ranges
        if ctx.deriv_coeffs is not None:
            with torch.no_grad():
                source, positions = ctx.saved_tensors
                g = grad_output.contiguous()
                lat = _cache.get(positions, ctx.deriv_coeffs)     # the derivative-tap lattice of the stacked positions
                # a = g on the out rows, b = source on the source rows: the source rows' positions (and wg on them)
                one_side = lat.apply_backward_rows_f32 if positions.dtype == torch.float32 else lat.apply_backward_rows
                grad_in, grad_source = one_side(g, ob, source, sb, positions, want_filtered=ctx.needs_input_grad[0])
                # a = source on the source rows, b = g on the out rows: the out rows' positions
                grad_out, _ = one_side(source, sb, g, ob, positions, want_filtered=False)
                grad_positions = torch.zeros_like(positions)
                grad_positions[sb:sb + sc] += grad_in
                grad_positions[ob:ob + oc] += grad_out
        elif ctx.needs_input_grad[0]:
            with torch.no_grad():
                lat = _cache.get(ctx.positions, ctx.coeffs)       # the forward's lattice (rebuilt if it was evicted since)
                grad_source = lat.apply_rows(grad_output.contiguous(), ob, sb, sc)
        return grad_source, grad_positions, None, None, None, None, None, None


class LatticeSliceAt(Function):
    """(out, mass) = the vertex array `values` of the built lattice `lat` sliced at the points x [nq, d] (in the build's
    units: already divided by the lengthscale): Lattice.locate + Lattice.slice_at, differentiable in x.

    The slice is piecewise linear in x; the backward is its exact derivative inside the simplex locate chose
    (query_grad.slice_at_backward: plx_slice_at_dots + plx_locate_pullback), returned in the dtype of
    x.  Once differentiable.  `mass` (locate's) carries no gradient.  `values` is a constant here, and a `values` that requires a
    gradient is refused: LatticeSliceAtValues differentiates it (the adjoint splat at the query points).  x and values are
    saved for the backward: changing either in place in between is an autograd error, not a wrong gradient."""

    @staticmethod
    def forward(ctx, x, values, lat, vd=None):
        if values.requires_grad:
            raise RuntimeError("LatticeSliceAt: values requires a gradient, but the adjoint splat at query points is not "
                               "built; detach values (only the query positions are differentiated)")
        query = lat.locate(x.detach())
        out = lat.slice_at(values, query, vd=vd)
        ctx.lat, ctx.query, ctx.vd = lat, query, vd
        ctx.save_for_backward(x, values)
        ctx.mark_non_differentiable(query.mass)
        return out, query.mass

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_mass):
        from . import query_grad
        x, values = ctx.saved_tensors
        grad_x = None
        if ctx.needs_input_grad[0]:
            g = grad_out.to(values.dtype).contiguous()
            grad_x = query_grad.slice_at_backward(ctx.lat, values, ctx.query, g, vd=ctx.vd).to(x.dtype)
        return grad_x, None, None, None


class LatticeSliceAtValues(Function):
    """LatticeSliceAt with a gradient for `values` too: (out, mass) = locate + slice_at, and in the backward
    grad_values = query_adjoint.slice_at_adjoint(grad_out) -- S*^T grad_out / (1 + 2^-d), one plan and one launch, no
    atomics -- beside the grad_x of LatticeSliceAt where x requires it.  Once differentiable; `mass`
    carries no gradient.  grad_values is [m, stride] like `values`, exact zeros in the stride padding."""

    @staticmethod
    def forward(ctx, x, values, lat, vd=None):
        query = lat.locate(x.detach())
        out = lat.slice_at(values.detach(), query, vd=vd)
        ctx.lat, ctx.query, ctx.vd = lat, query, out.shape[1]
        ctx.save_for_backward(x, values)
        ctx.mark_non_differentiable(query.mass)
        return out, query.mass

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_mass):
        from . import query_adjoint, query_grad
        x, values = ctx.saved_tensors
        g = grad_out.to(values.dtype).contiguous()
        grad_x = grad_values = None
        if ctx.needs_input_grad[0]:
            grad_x = query_grad.slice_at_backward(ctx.lat, values, ctx.query, g, vd=ctx.vd).to(x.dtype)
        if ctx.needs_input_grad[1]:
            grad_values = query_adjoint.slice_at_adjoint(ctx.lat, g, ctx.query)
            if grad_values.shape[0] != values.shape[0]:       # a values buffer with spare rows: they were not read
                grad_values = torch.cat([grad_values, grad_values.new_zeros(values.shape[0] - grad_values.shape[0],
                                                                             grad_values.shape[1])])
        return grad_x, grad_values, None, None


class LatticeQueryProduct(Function):
    """(K_q src, mass) for the built lattice `lat`, src [n, vd] and the points x [nq, d] (in the build's units):
    Lattice.blurred + locate + slice_at.  Backward: grad_src = query_adjoint.apply_at_t(grad_out), the exact transpose of
    the forward map (S_X blur_t S*^T / (1 + 2^-d)), and grad_x as in LatticeSliceAt from the blurred buffer the forward
    kept.  One plan per backward.  Once differentiable; `mass` carries no gradient."""

    @staticmethod
    def forward(ctx, lat, src, x):
        values, vd = lat.blurred(src.detach())
        query = lat.locate(x.detach())
        out = lat.slice_at(values, query, vd=vd)
        ctx.lat, ctx.query, ctx.vd, ctx.values = lat, query, vd, values
        ctx.save_for_backward(x)
        ctx.src_dtype = src.dtype
        ctx.mark_non_differentiable(query.mass)
        return out, query.mass

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_mass):
        from . import query_adjoint, query_grad
        (x,) = ctx.saved_tensors
        g = grad_out.to(ctx.src_dtype).contiguous()
        grad_src = query_adjoint.apply_at_t(ctx.lat, g, ctx.query) if ctx.needs_input_grad[1] else None
        grad_x = None
        if ctx.needs_input_grad[2]:
            grad_x = query_grad.slice_at_backward(ctx.lat, ctx.values, ctx.query, g, vd=ctx.vd).to(x.dtype)
        return None, grad_src, grad_x


def rows_route(device_type, dtype, dim, hook, requires_grad, enabled=True, columns=None, min_columns=1, f64=False,
               grad_f64=False, grad_f32=False):
    """Whether K(xin, xout) @ V goes through the native row-range product: a CUDA fp32 2-D right-hand side -- or, with
    f64=True (RectangularLazyLattice.native_rows_f64), a float64 one --, no test hook / foreign filter installed
    (LatticeFilterGeneral.method), no gradient wanted for the positions, the route switched on
    (RectangularLazyLattice.native_rows) and, where the caller says how many columns V has, at least `min_columns` of them
    (RectangularLazyLattice.native_min_columns).  Everything else takes the padded square filter.

    grad_f64=True (RectangularLazyLattice.native_rows_grad_f64) asks the other question: whether a product whose positions
    DO want a gradient goes through the native route with its native float64 position gradient.  That admits only a CUDA
    float64 2-D right-hand side with requires_grad set, no hook, the route switched on; the width gate does not apply
    (it was measured for the fp32 forward).

    grad_f32=True (RectangularLazyLattice.native_rows_grad) asks the same of the native fp32 position gradient: only a CUDA
    float32 2-D right-hand side with requires_grad set, no hook, the route switched on; no width gate either."""
    if grad_f32:
        return bool(enabled and device_type == "cuda" and dtype == torch.float32 and dim == 2 and hook is None
                    and requires_grad)
    if grad_f64:
        return bool(enabled and device_type == "cuda" and dtype == torch.float64 and dim == 2 and hook is None
                    and requires_grad)
    dtype_ok = dtype == torch.float32 or (bool(f64) and dtype == torch.float64)
    return bool(enabled and device_type == "cuda" and dtype_ok and dim == 2 and hook is None
                and not requires_grad and (columns is None or columns >= min_columns))


def _lattice_matvec(rhs, positions, dkernel):
    """K(positions) @ rhs through the autograd op; the one place the operator classes reach the native filter."""
    return LatticeFilterGeneral.apply(rhs, positions, dkernel)


class SquareLazyLattice(LazyTensor):
    """K(x, x), known through its action only (py:127-140): symmetric by declaration (its transpose is itself,
    py:137-138) and with a unit diagonal by declaration (py:139-140), whatever the lattice actually computes.  The
    declared diagonal has a true counterpart, the K_ii the product forms (Lattice.diag, plx_diag / plx_diag_f64): with the
    class switch `true_diag` on, diag() of a CUDA operator on a plain build returns it."""

    true_diag = False      # class switch: diag() returns the operator's own diagonal where the native call serves it

    def __init__(self, x, dkernel=None, symmetrized=False):
        super().__init__(x, dkernel=dkernel, symmetrized=symmetrized)
        self.x, self.dkernel, self.symmetrized = x, dkernel, bool(symmetrized)

    def _size(self):
        n = self.x.shape[-2]
        return torch.Size((n, n))

    def _matmul(self, V):
        if self.symmetrized and V.dtype == torch.float64:
            # K_s = (K + K^T) / 2 on the forward-tap lattice (Lattice.apply_sym): symmetric to rounding, so the
            # declaration below is then true of what is computed.  No autograd through this product.
            if not (V.is_cuda and V.dim() == 2 and self.x.dtype == torch.float64):
                raise TypeError("SquareLazyLattice(symmetrized=True) serves CUDA float64 2-D right-hand sides on float64 "
                                "positions only")
            x = self.x.detach()
            x = x if x.is_contiguous() else carry_hint(x.contiguous(), x)
            return _cache.get(x, self.dkernel.get_coeffs()).apply_sym(V.detach())
        return _lattice_matvec(V, self.x, self.dkernel)

    def _transpose_nonbatch(self):
        return self

    def diag(self):
        x = self.x
        if self.true_diag and x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64):
            xc = x.detach()
            xc = xc if xc.is_contiguous() else carry_hint(xc.contiguous(), xc)
            lat = _cache.get(xc, self.dkernel.get_coeffs())      # the forward-tap lattice of the products
            if lat.accepts_rows():
                return lat.diag(dtype=x.dtype)
        return x.new_ones(x.shape[:-1])


class RectangularLazyLattice(LazyTensor):
    """K(xin, xout) for two different point sets (prediction), py:142-160: the right-hand side lives on `xout`; it is
    extended by zeros over `xin`, ONE square filter runs over the stacked points [xout; xin], and the rows that belong to
    `xin` are returned.

    native_rows: where rows_route() allows it, and the lattice of the stacked points is a plain single-shard build, the
    product runs as plx_apply_rows on that lattice instead -- the rows of `xout` are splatted, the rows of `xin` sliced,
    nothing is padded or thrown away -- and the transposed operator works on the SAME lattice with the two ranges swapped
    (it does not build [xin; xout] again).  False: the padded path, always.

    native_min_columns: the route is taken from this many columns of V on.  Measured at N = 1e6 + 2.5e5, d = 8
    (profiles/rows_measured.md): at 101 columns (a prediction split) the native product is 10 % faster than the padded one
    and needs 1.25 GB less; at 11 and at 1 column its vertex-gather splat loses to the square stages' tuned narrow kernels
    (0.89 against 0.68 ms, 0.59 against 0.24 ms).  The crossover between 11 and 101 has not been located, so everything
    below the measured winning width keeps the padded path.

    native_rows_f64: whether a float64 V takes the native route too (plx_apply_rows_f64; the same width gate).  The
    native and the padded float64 products are equal as values, so the switch changes time and
    memory only.  It is off until the native product has been measured no slower than the padded one at 101 columns in
    both directions (profiles/rows_f64_measured.md: not measured yet).

    native_rows_grad_f64: whether a float64 2-D V whose positions WANT a gradient takes the native route as well, with the
    position gradient as two one-sided native calls of half the padded width (LatticeRowsProduct)
    instead of one padded square gradient.  Both lattices (the kernel's taps and the derivative taps, on the stacked
    points) must accept rows and Lattice.backward_rows_f64_ok must hold; native_min_columns does not apply (it was
    measured for the fp32 forward).  The two routes agree to rounding.  Off until the native route has been measured no
    slower than the padded one at every shape of tools/rows_backward_f64_time.py
    (profiles/rows_backward_f64_measured.md).

    native_rows_grad: the same for a float32 2-D V whose positions want a gradient (Lattice.apply_backward_rows_f32,
    DESIGN.md section 22): both lattices must accept rows and Lattice.backward_rows_ok must hold; no width gate.  The two
    routes agree to rounding.  On only if the native route is no slower than the padded one at every shape of
    tools/rows_backward_time.py (profiles/rows_backward_measured.md says which it is, and which shapes lose)."""

    native_rows = True
    native_min_columns = 101
    native_rows_f64 = False
    native_rows_grad_f64 = False
    native_rows_grad = False

    def __init__(self, xin, xout, dkernel=None):
        super().__init__(xin, xout, dkernel=dkernel)
        self.xin, self.xout, self.dkernel = xin, xout, dkernel

    def _size(self):
        return torch.Size((*self.xin.shape[:-1], self.xout.shape[-2]))

    def _matmul(self, V):
        n_out, n_in = self.xout.shape[-2], self.xin.shape[-2]
        assert V.shape[-2] == n_out, f"mismatched shapes? {V.shape, self.xout.shape}"
        wants_grad = torch.is_grad_enabled() and (self.xin.requires_grad or self.xout.requires_grad)
        if rows_route(V.device.type, V.dtype, V.dim(), LatticeFilterGeneral.method, wants_grad, type(self).native_rows,
                      V.shape[-1], type(self).native_min_columns, f64=type(self).native_rows_f64):
            base, swapped = self.__dict__.get("_rows_base", (self, False))
            stacked = base._stacked_points()                       # [base.xout; base.xin]: one lattice for both directions
            coeffs = self.dkernel.get_coeffs()
            lat = _cache.get(stacked, coeffs)
            if lat.accepts_rows():
                nb_out = base.xout.shape[-2]
                src_begin, out_begin = (nb_out, 0) if swapped else (0, nb_out)
                return LatticeRowsProduct.apply(V, stacked, coeffs, lat, src_begin, out_begin, n_in)
        elif ((type(self).native_rows_grad_f64
               and rows_route(V.device.type, V.dtype, V.dim(), LatticeFilterGeneral.method, wants_grad, type(self).native_rows,
                              grad_f64=True)
               and Lattice.backward_rows_f64_ok(V.shape[-1], self.xin.shape[-1]))
              or (type(self).native_rows_grad
                  and rows_route(V.device.type, V.dtype, V.dim(), LatticeFilterGeneral.method, wants_grad,
                                 type(self).native_rows, grad_f32=True)
                  and Lattice.backward_rows_ok(V.shape[-1], self.xin.shape[-1]))):
            base, swapped = self.__dict__.get("_rows_base", (self, False))
            stacked = base._stacked_points()                       # the concatenation WITH its gradient history
            coeffs = self.dkernel.get_coeffs()
            lat = _cache.get(stacked, coeffs)
            dlat = _cache.get(stacked, self.dkernel.get_deriv_coeffs())
            if lat.accepts_rows() and dlat.accepts_rows():
                nb_out = base.xout.shape[-2]
                src_begin, out_begin = (nb_out, 0) if swapped else (0, nb_out)
                return LatticeRowsProduct.apply(V, stacked, coeffs, lat, src_begin, out_begin, n_in, self.dkernel)
        stacked_rhs = torch.nn.functional.pad(V, (0, 0, 0, n_in))          # zero rows for the points of xin
        return _lattice_matvec(stacked_rhs, self._stacked_points(), self.dkernel)[..., n_out:, :]

    def _stacked_points(self):
        """[xout; xin].  Without a gradient to carry, the stacked tensor is made once per operator (and per state of its
        two inputs): a fresh concatenation on every product is a fresh lattice-cache key, i.e. one lattice build per product
        (measured, N = 1e6 + 2.5e5 points: 1.5 of the 9.8 ms of every K(x*, x) @ V on the same operator)."""
        if torch.is_grad_enabled() and (self.xin.requires_grad or self.xout.requires_grad):
            return torch.cat((self.xout, self.xin), dim=-2)
        key = (self.xin._version, self.xout._version)
        hit = self.__dict__.get("_stacked")
        if hit is None or hit[0] != key:
            hit = (key, stack_hint(torch.cat((self.xout.detach(), self.xin.detach()), dim=-2), (self.xout, self.xin)))
            self.__dict__["_stacked"] = hit
        return hit[1]

    def _transpose_nonbatch(self):
        t = type(self)(self.xout, self.xin, self.dkernel)
        base, swapped = self.__dict__.get("_rows_base", (self, False))
        t.__dict__["_rows_base"] = (base, not swapped)             # the native route serves it from base's lattice
        return t


class LatticeAccelerated(Kernel):
    """A stationary kernel, given as a differentiable profile in the squared distance, evaluated through the
    permutohedral lattice (py:183-200).  ARD lengthscales divide the inputs before they reach the lattice (py:198-200);
    the diagonal is reported as ones (py:193-195); the diagonal the lattice computes is Lattice.diag (and
    SquareLazyLattice.diag() under its `true_diag` switch)."""

    has_lengthscale = True

    def __init__(self, kernel_fn, *args, order=2, **kwargs):
        super().__init__(*args, **kwargs)
        self.dkernel_fn = DiscretizedKernelFN(kernel_fn, order)

    @staticmethod
    def _same_points(a, b):
        """The reference decides square vs rectangular by comparing the two tensors element by element on every call
        (py:197, one device synchronisation); identical objects / storage are recognised without that."""
        if a is b:
            return True
        if a.shape != b.shape:
            return False
        return a.data_ptr() == b.data_ptr() or bool(torch.equal(a, b))

    def forward(self, x1, x2, diag=False, **params):
        if diag:
            return x1.new_ones(x1.shape[:-1])
        scaled1 = position_hint(x1.div(self.lengthscale), x1, scale_of=getattr(self, "raw_lengthscale", None))
        if self._same_points(x1, x2):
            return SquareLazyLattice(scaled1, self.dkernel_fn)
        scaled2 = position_hint(x2.div(self.lengthscale), x2, scale_of=getattr(self, "raw_lengthscale", None))
        return RectangularLazyLattice(scaled1, scaled2, self.dkernel_fn)


# The factories record the profile's name on the kernel they return (`profile`, exact.PROFILES), so that
# exact.exact_twin can find the exact kernel a lattice kernel approximates; a kernel built from any other callable has none.
def _lattice_kernel_factory(profile, default_order, name):
    def make(*args, order=default_order, **kwargs):
        k = LatticeAccelerated(profile, *args, order=order, **kwargs)
        k.profile = name
        return k
    return make


RBFLattice = _lattice_kernel_factory(rbf, 2, "rbf")             # py:247-248
RBFLattice.__name__ = "RBFLattice"
BilateralKernel = RBFLattice                                    # py:250-251


def MaternLattice(*args, nu=1.5, order=3, **kwargs):            # py:253-254
    k = LatticeAccelerated(lambda d2: Matern.apply(d2, nu), *args, order=order, **kwargs)
    k.profile = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}.get(nu)
    return k
