"""Device lattice handle + the reference's `filter(src, ref, coeffs)` boundary.

`filter` is the drop-in for the one native symbol of the reference
(gpytorch_lattice_kernel/cpp/lattice.cpp:6-16, cuda/permutohedral_cuda.cpp:12-22):
same argument order, shapes, dtype and return value.  `Lattice` is the staged
form (build once, apply many times) that the CG loop and the backward pass use.

torch is plumbing here: device memory, the current stream, nothing else.
"""
import ctypes

import numpy as np
import torch

from . import _native as nv


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _taps_array(coeffs):
    if isinstance(coeffs, torch.Tensor):
        coeffs = coeffs.detach().to("cpu", torch.float32).numpy()
    taps = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1)
    if taps.size % 2 != 1:
        raise ValueError(f"coeffs must have an odd number of taps, got {taps.size}")
    return taps


def _check_f32_cuda(t, name, ndim=2, f64_ok=False):
    """f64_ok: the call has a float64 form (the stages, the product and the rows calls, not the build)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (HIP) tensor; this build has no CPU path")
    if t.dtype != torch.float32 and not (f64_ok and t.dtype == torch.float64):
        raise TypeError(f"{name} must be float32{' or float64' if f64_ok else ''}, got {t.dtype}")
    if t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {tuple(t.shape)}")


def _positions_f32(ref, name="ref"):
    """The positions a lattice is built on: float32.  float64 positions are ROUNDED to float32 -- the float64 product runs
    on the fp32 build's lattice (its error against the exact kernel is the lattice's, not the embedding's), so one build
    serves both precisions."""
    _check_f32_cuda(ref, name, f64_ok=True)
    return ref if ref.dtype == torch.float32 else ref.to(torch.float32)


class LatticeQuery:
    """Where nq points that are not the build's sit in a built lattice (Lattice.locate): vid [d+1, nq] int32, the vertex id
    of every simplex corner in the numbering of build `build_id` of that lattice, -1 where the corner is not one of its
    vertices; weight [d+1, nq] float32, the barycentric weights; mass [nq] float32 (None when not asked for), the sum of
    the weights of the corners found: 1 where the whole simplex exists, 0 where the lattice knows nothing of the point;
    x [nq, d] float32 (None when built by hand without it), the contiguous positions locate read -- what the position
    gradient (simplex_gp_amd.query_grad) recomputes the simplex from.  x is NOT a copy: where the caller's tensor was
    contiguous float32 already it is that tensor, and changing it in place after locate makes the pull-back recompute
    another simplex than the one vid and weight describe.  Clone before locate if the positions are to be overwritten."""
    __slots__ = ("vid", "weight", "mass", "nq", "build_id", "x")

    def __init__(self, vid, weight, mass, nq, build_id, x=None):
        self.vid, self.weight, self.mass, self.nq, self.build_id, self.x = vid, weight, mass, int(nq), int(build_id), x


class Lattice:
    """One permutohedral lattice on one GPU.

    build(ref, coeffs) fixes the structure (vertices, barycentric weights,
    blur neighbour table, splat CSR); apply(src) is one K.v MVM on it.
    Not thread-safe (ping-pong workspace), same as documented in plx.h.
    """

    def __init__(self, device=None):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self._h = ctypes.c_void_p()
        nv.check(nv.lib().plx_create(self.device.index, ctypes.byref(self._h)), "plx_create")
        self._ref = None          # keeps the positions alive while kernels may still read them
        self.taps = None
        self._perm_cache = None
        self._own_begin = 0
        self.lattice_rows = False
        self._dot_work = None
        self._dot_work64 = None   # float64 partial sums of apply_affine(want_dot=True) in double: grow-only, separate
        self.build_id = 0         # counts the builds of this object (holders of per-build data compare it)
        self._merged = False      # built by build_local + build_merge (one rank's rows of a sharded lattice)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            nv.lib().plx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- structure --------------------------------------------------------
    def build(self, ref, coeffs, shard=None, reuse_order=False):
        """shard = (index, count): this process splats / slices block `index` of the
        `count` contiguous near-equal row blocks (distributed.shard_bounds); None = all rows.
        reuse_order=True: `ref` is the previous build's positions re-scaled a little (a lengthscale that moved): keep the
        lattice order of the points (plx_set_reuse_order: the order passes of the build are skipped; the result is the
        cold build's up to the order of the fp32 sums inside a vertex row).  Ignored when no order of that shape exists."""
        _check_f32_cuda(ref, "ref")
        ref = ref.contiguous()
        taps = _taps_array(coeffs)
        n, d = ref.shape
        index, count = (0, 1) if shard is None else shard
        if reuse_order:
            nv.check(nv.lib().plx_set_reuse_order(self._h, 1), "plx_set_reuse_order")
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_build(self._h, ctypes.c_void_p(ref.data_ptr()), n, d,
                                    taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), taps.size,
                                    index, count, _stream_ptr(self.device))
        nv.check(rc, "plx_build")
        self.build_id += 1
        self._merged = False
        self._ref = ref
        self.taps = taps
        self._perm_cache = None
        base, extra = divmod(n, count)
        self._own_begin = index * base + min(index, extra)
        return self

    def filter_once(self, src, ref, coeffs, out=None):
        """plx_filter on this lattice's buffers: build for `ref`, one MVM of `src`, in one native call.  The build knows
        the lattice serves a single MVM and leaves out what only pays back over several (vertex renumbering, axis-pair
        tables); the lattice stays usable afterwards like one built by build()."""
        _check_f32_cuda(ref, "ref")
        ref = ref.contiguous()
        taps = _taps_array(coeffs)
        n, d = ref.shape
        src = self._src(src, n)
        vd = src.shape[1]
        if out is None:
            out = torch.empty((n, vd), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_filter(self._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(ref.data_ptr()), n, d, vd,
                                     taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), taps.size,
                                     ctypes.c_void_p(out.data_ptr()), _stream_ptr(self.device))
        nv.check(rc, "plx_filter")
        self.build_id += 1
        self._merged = False
        self._ref, self.taps, self._perm_cache, self._own_begin = ref, taps, None, 0
        return out

    # -- sharded build: local stage / key exchange / merge ---------------------
    def build_local(self, ref_local, coeffs):
        """Stage 1 of a sharded build: structure of this rank's own rows only.
        Returns the rank's vertex keys as an int32 tensor [m_local, key_words]."""
        _check_f32_cuda(ref_local, "ref_local")
        ref_local = ref_local.contiguous()
        taps = _taps_array(coeffs)
        n, d = ref_local.shape
        L = nv.lib()
        with torch.cuda.device(self.device):
            rc = L.plx_build_local(self._h, ctypes.c_void_p(ref_local.data_ptr()), n, d,
                                   taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), taps.size,
                                   _stream_ptr(self.device))
        nv.check(rc, "plx_build_local")
        self.build_id += 1
        self._merged = True
        self._ref, self.taps, self._perm_cache, self._own_begin = ref_local, taps, None, 0
        keys = torch.empty((int(L.plx_local_vertices(self._h)), int(L.plx_key_words(d))), dtype=torch.int32,
                           device=self.device)
        with torch.cuda.device(self.device):
            rc = L.plx_copy_local_keys(self._h, ctypes.c_void_p(keys.data_ptr()), _stream_ptr(self.device))
        nv.check(rc, "plx_copy_local_keys")
        return keys

    def build_merge(self, all_keys, counts, rank, total_points=0):
        """Stage 2: all ranks' keys concatenated in rank order ([sum(counts), key_words] int32); total_points = rows of
        all ranks together (feeds the vertex-numbering choice only; 0 = unknown)."""
        all_keys = all_keys.contiguous()
        assert all_keys.is_cuda and all_keys.dtype == torch.int32 and all_keys.shape[0] == sum(counts)
        arr = (ctypes.c_int64 * len(counts))(*[int(c) for c in counts])
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_build_merge(self._h, ctypes.c_void_p(all_keys.data_ptr()), arr, len(counts), rank,
                                          int(total_points), _stream_ptr(self.device))
        nv.check(rc, "plx_build_merge")
        return self

    @property
    def order_age(self):
        """Builds since the point order was computed from the positions themselves (0: by the last build; -1: none)."""
        return int(nv.lib().plx_order_age(self._h))

    @property
    def n(self):
        return int(nv.lib().plx_num_points(self._h))

    @property
    def n_owned(self):
        return int(nv.lib().plx_num_owned(self._h))

    @property
    def m(self):
        return int(nv.lib().plx_num_vertices(self._h))

    @property
    def d(self):
        return int(nv.lib().plx_dim(self._h))

    @property
    def order(self):
        return int(nv.lib().plx_order(self._h))

    @property
    def device_bytes(self):
        return int(nv.lib().plx_device_bytes(self._h))

    # -- row order ----------------------------------------------------------
    def shard_perm(self):
        """int64 device tensor: caller row (within this shard) of the i-th row in lattice order."""
        if self._perm_cache is None:
            raw = torch.empty(self.n, dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                rc = nv.lib().plx_copy_point_perm(self._h, ctypes.c_void_p(raw.data_ptr()), _stream_ptr(self.device))
            nv.check(rc, "plx_copy_point_perm")
            begin = self._own_begin        # rows of this shard occupy the same index range in both orders
            self._perm_cache = raw[begin:begin + self.n_owned].to(torch.int64) - begin
        return self._perm_cache

    def set_lattice_row_order(self, on=True):
        """on: splat/slice/apply take and return rows in lattice order (no per-MVM permutation)."""
        nv.check(nv.lib().plx_set_row_order(self._h, 1 if on else 0), "plx_set_row_order")
        self.lattice_rows = bool(on)

    def to_lattice_order(self, t):
        return t.index_select(0, self.shard_perm())

    def from_lattice_order(self, t):
        out = torch.empty_like(t)
        out.index_copy_(0, self.shard_perm(), t)
        return out

    def set_timing(self, on=True):
        nv.check(nv.lib().plx_set_timing(self._h, 1 if on else 0), "plx_set_timing")

    def reference_growth_info(self):
        """What the replay of the reference CPU path's table-growth quirk found for this build (plx_tune
        "reference_growth"): {"replayed", "m_reference", "dropped", "invisible", "blur_miss", "inexact"}."""
        buf = (ctypes.c_int64 * 6)()
        nv.check(nv.lib().plx_reference_growth_info(self._h, buf), "plx_reference_growth_info")
        return {"replayed": bool(buf[0]), "m_reference": int(buf[1]), "dropped": int(buf[2]), "invisible": int(buf[3]),
                "blur_miss": bool(buf[4]), "inexact": bool(buf[5])}

    def build_times_ms(self):
        buf = (ctypes.c_float * 6)()
        nv.check(nv.lib().plx_build_times(self._h, buf), "plx_build_times")
        return dict(zip(("embed", "insert", "number", "ids", "neighbours", "csr"), list(buf)))

    def _last_kernels(self, fn, cap):
        """What the C call `fn` reports, "a=x+y;b=z", as {"a": ["x", "y"], "b": ["z"]}."""
        buf = ctypes.create_string_buffer(cap)
        nv.check(getattr(nv.lib(), fn)(self._h, buf, cap), fn)
        out = {}
        for part in buf.value.decode().split(";"):
            k, _, names = part.partition("=")
            out[k] = [x for x in names.split("+") if x]
        return out

    def stage_kernels(self, vd=None):
        """Kernels launched by the last splat / blur / slice on this lattice: {"splat": [...], "blur_axis": [...],
        "slice": [...]} (names as rocprofv3 shows them, without template arguments)."""
        return self._last_kernels("plx_last_kernels", 512)

    def prepare(self, vd=1):
        """Build now every table an MVM with vd columns will read (otherwise the first such MVM builds them)."""
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_prepare(self._h, int(vd), _stream_ptr(self.device))
        nv.check(rc, "plx_prepare")
        return self

    def tune(self, key, value):
        """Switch a kernel variant for THIS lattice only, from its next call until its next build (plx_lattice_tune;
        the process defaults -- plx_tune -- are what every build starts from)."""
        nv.check(nv.lib().plx_lattice_tune(self._h, key.encode(), int(value)), "plx_lattice_tune")
        return self

    @property
    def block_rows(self):
        """Rows of the block tables (0: not built yet -- see prepare() -- or the lattice uses the vertex-sorted CSR path)."""
        return int(nv.lib().plx_block_rows(self._h))

    def apply_times_ms(self):
        """Stage times of the last apply(): dict(splat, blur, slice) in ms (blur = all d+1 launches)."""
        cap = 8
        buf = (ctypes.c_float * cap)()
        cnt = ctypes.c_int(0)
        nv.check(nv.lib().plx_apply_times(self._h, buf, cap, ctypes.byref(cnt)), "plx_apply_times")
        t = list(buf)[:cnt.value]
        if len(t) != 3:
            return None
        return {"splat": t[0], "blur": t[1], "slice": t[2]}

    # -- stages -----------------------------------------------------------
    def _src(self, src, rows, f64_ok=False):
        _check_f32_cuda(src, "src", f64_ok=f64_ok)
        if src.shape[0] != rows:
            raise ValueError(f"Incompatible shapes {tuple(src.shape)}, expected {rows} rows")
        return src.contiguous()

    # The stages and the product dispatch on the dtype of the values: float32 runs the kernels the build was made for,
    # float64 (plx_*_f64) the same structure with the fp32 weights and taps converted exactly and every sum in double.
    # float64 rows are always in the caller's order, on plain single-shard builds only (PlxError otherwise).
    @staticmethod
    def values_stride(vd, dtype=torch.float32):
        """Elements per vertex row of a values buffer: vd rounded up to 4 floats, or to 2 doubles, when vd > 1."""
        if dtype == torch.float64:
            return int(nv.lib().plx_values_stride_f64(vd))
        return int(nv.lib().plx_values_stride(vd))

    def new_values(self, vd, dtype=torch.float32):
        """Vertex accumulator [m, values_stride(vd, dtype)]; columns >= vd are zero padding."""
        return torch.empty((self.m, self.values_stride(vd, dtype)), dtype=dtype, device=self.device)

    def splat(self, src, values=None):
        src = self._src(src, self.n_owned, f64_ok=True)
        vd = src.shape[1]
        f64 = src.dtype == torch.float64
        if values is None:
            values = self.new_values(vd, src.dtype)
        elif values.dtype != src.dtype:
            raise TypeError(f"values must be {src.dtype} like src, got {values.dtype}")
        fn, name = (nv.lib().plx_splat_f64, "plx_splat_f64") if f64 else (nv.lib().plx_splat, "plx_splat")
        with torch.cuda.device(self.device):
            rc = fn(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(values.data_ptr()),
                    _stream_ptr(self.device))
        nv.check(rc, name)
        return values

    def splat_onehot(self, points, nb, values, vd=None):
        """values[:, b] = S^T e_p for p = points[b] (device int32, lattice-order point indices), b < nb; zero elsewhere."""
        vd = values.shape[1] if vd is None else vd
        assert values.shape[1] == self.values_stride(vd) and values.is_contiguous() and points.dtype == torch.int32
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_splat_onehot(self._h, ctypes.c_void_p(points.data_ptr()), int(nb), vd,
                                           ctypes.c_void_p(values.data_ptr()), _stream_ptr(self.device))
        nv.check(rc, "plx_splat_onehot")
        return values

    def filter_onehot(self, points, nb, values, scratch, out, vd=None, sparse=True, frontier=None):
        """out[:, b] = K e_p for p = points[b] (device int32, lattice-order point indices), b < nb <= 16: splat_onehot +
        blur + slice in one call; sparse=True runs them on the frontier of the columns' non-zero vertex rows
        (plx_filter_onehot).  values / scratch: two [m, values_stride(vd)] buffers (clobbered); out: [n, vd], rows in
        the order set_lattice_row_order() says; frontier (optional device int32 [1]) receives the vertex rows the last
        blur axis worked on."""
        vd = out.shape[1] if vd is None else vd
        _check_f32_cuda(values, "values"); _check_f32_cuda(scratch, "scratch"); _check_f32_cuda(out, "out")
        assert values.shape[1] == self.values_stride(vd) and values.is_contiguous() and scratch.shape == values.shape
        assert scratch.is_contiguous() and values.shape[0] >= self.m and points.dtype == torch.int32 and points.numel() >= nb
        assert out.is_contiguous() and out.shape == (self.n_owned, vd)
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_filter_onehot(self._h, ctypes.c_void_p(points.data_ptr()), int(nb), vd,
                                            ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
                                            ctypes.c_void_p(out.data_ptr()), 1 if sparse else 0,
                                            ctypes.c_void_p(frontier.data_ptr()) if frontier is not None else None,
                                            _stream_ptr(self.device))
        nv.check(rc, "plx_filter_onehot")
        return out

    def blur(self, values, scratch=None, vd=None):
        """Returns the tensor holding the blurred values (either `values` or `scratch`).
        `values` is [m, values_stride(vd)]; vd defaults to its width."""
        _check_f32_cuda(values, "values", f64_ok=True)
        vd = values.shape[1] if vd is None else vd
        assert values.shape[1] == self.values_stride(vd, values.dtype) and values.is_contiguous()
        if values.shape[0] < self.m:
            raise ValueError(f"values has {values.shape[0]} rows, the lattice {self.m} vertices")
        if scratch is None:
            scratch = torch.empty_like(values)
        elif scratch.numel() < values.numel() or not scratch.is_contiguous() or scratch.dtype != values.dtype:
            raise ValueError("scratch must be a contiguous buffer of the values' dtype, at least as large as values")
        flag = ctypes.c_int(0)
        f64 = values.dtype == torch.float64
        fn, name = (nv.lib().plx_blur_f64, "plx_blur_f64") if f64 else (nv.lib().plx_blur, "plx_blur")
        with torch.cuda.device(self.device):
            rc = fn(self._h, ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), vd,
                    ctypes.byref(flag), _stream_ptr(self.device))
        nv.check(rc, name)
        return scratch if flag.value else values

    def slice(self, values, out=None, vd=None):
        _check_f32_cuda(values, "values", f64_ok=True)
        vd = values.shape[1] if vd is None else vd
        assert values.shape[1] == self.values_stride(vd, values.dtype) and values.is_contiguous()
        if out is None:
            out = torch.empty((self.n_owned, vd), dtype=values.dtype, device=self.device)
        elif out.dtype != values.dtype:
            raise TypeError(f"out must be {values.dtype} like values, got {out.dtype}")
        f64 = values.dtype == torch.float64
        fn, name = (nv.lib().plx_slice_f64, "plx_slice_f64") if f64 else (nv.lib().plx_slice, "plx_slice")
        with torch.cuda.device(self.device):
            rc = fn(self._h, ctypes.c_void_p(values.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                    _stream_ptr(self.device))
        nv.check(rc, name)
        return out

    def apply(self, src, out=None):
        """One MVM: out = slice(blur(splat(src))) on the lattice's own workspace, in the dtype of `src` (float64: on a
        workspace of doubles that the first such call allocates)."""
        src = self._src(src, self.n_owned, f64_ok=True)
        vd = src.shape[1]
        if out is None:
            out = torch.empty((self.n_owned, vd), dtype=src.dtype, device=self.device)
        elif out.dtype != src.dtype:
            raise TypeError(f"out must be {src.dtype} like src, got {out.dtype}")
        f64 = src.dtype == torch.float64
        fn, name = (nv.lib().plx_apply_f64, "plx_apply_f64") if f64 else (nv.lib().plx_apply, "plx_apply")
        with torch.cuda.device(self.device):
            rc = fn(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                    _stream_ptr(self.device))
        nv.check(rc, name)
        return out

    def f64_kernels(self):
        """Kernels launched by the last float64 splat / blur / slice (or apply) on this lattice: {"splat": [...],
        "blur_axis": [...], "slice": [...]}; stage_kernels() goes on naming the fp32 stages."""
        return self._last_kernels("plx_last_f64_kernels", 256)

    # -- the transposed and symmetrised float64 products (plx_*_t_f64 / plx_*_sym_f64) ------
    # K is not symmetric (the axis blurs do not commute).  K^T runs the axes in reverse with mirrored taps; K_s = (K + K^T) / 2
    # advances both blur chains in each of its d + 1 launches.  These methods are float64 only; the fp32 forms have names of
    # their own (blur_t_f32 ... below) and run one general kernel family, since the plain fp32 blur's families carry
    # order-dependent pair stencils.
    @staticmethod
    def _f64_only(t, name, what):
        if isinstance(t, torch.Tensor) and t.dtype != torch.float64:
            raise TypeError(f"{what} is served in float64 only (the transposed and symmetrised lattice products have no "
                            f"fp32 form), got {name} of {t.dtype}")

    def blur_t(self, values, scratch=None, vd=None):
        """The adjoint of the float64 blur(): axes d .. 0, mirrored taps (plx_blur_t_f64).  Returns the tensor that holds
        the result (either `values` or `scratch`), as blur() does."""
        return self._blur_t(torch.float64, "plx_blur_t_f64", lambda t, name: self._f64_only(t, name, "blur_t"),
                            "buffer of the values' dtype", values, scratch, vd)

    def _blur_t(self, dtype, symbol, refuse, scratch_is, values, scratch, vd):
        """The body of blur_t (float64) and blur_t_f32 (float32): `symbol` is the library's call for `dtype`, `refuse`
        the public method's refusal of the other dtype, `scratch_is` its words for the scratch buffer."""
        refuse(values, "values")
        _check_f32_cuda(values, "values", f64_ok=dtype == torch.float64)
        vd = values.shape[1] if vd is None else vd
        assert values.shape[1] == self.values_stride(vd, dtype) and values.is_contiguous()
        if values.shape[0] < self.m:
            raise ValueError(f"values has {values.shape[0]} rows, the lattice {self.m} vertices")
        if scratch is None:
            scratch = torch.empty_like(values)
        elif scratch.numel() < values.numel() or not scratch.is_contiguous() or scratch.dtype != values.dtype:
            raise ValueError(f"scratch must be a contiguous {scratch_is}, at least as large as values")
        flag = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            rc = getattr(nv.lib(), symbol)(self._h, ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), vd,
                                           ctypes.byref(flag), _stream_ptr(self.device))
        nv.check(rc, symbol)
        return scratch if flag.value else values

    def blur_sym(self, values, work=None, vd=None):
        """0.5 * (blur(values) + blur_t(values)) in d + 1 launches that advance both chains (plx_blur_sym_f64).  `values`
        [m, values_stride(vd)] float64 is clobbered; `work`: a contiguous float64 buffer of at least
        plx_blur_sym_work_doubles elements (allocated when None).  Returns an [m, stride] tensor that views `values` or
        `work`, wherever the result lies."""
        return self._blur_sym(torch.float64, "plx_blur_sym_f64", "plx_blur_sym_work_doubles", "blur_sym",
                              lambda t, name: self._f64_only(t, name, "blur_sym"), values, work, vd)

    def _blur_sym(self, dtype, symbol, work_symbol, what, refuse, values, work, vd):
        """The body of blur_sym (float64) and blur_sym_f32 (float32): `symbol` and `work_symbol` are the library's call and
        its work-size function for `dtype`, `what` the public method's name, `refuse` its refusal of the other dtype."""
        refuse(values, "values")
        _check_f32_cuda(values, "values", f64_ok=dtype == torch.float64)
        vd = values.shape[1] if vd is None else vd
        stride = self.values_stride(vd, dtype)
        assert values.shape[1] == stride and values.is_contiguous()
        if values.shape[0] < self.m:
            raise ValueError(f"values has {values.shape[0]} rows, the lattice {self.m} vertices")
        need = int(getattr(nv.lib(), work_symbol)(self._h, vd))
        if need < 0:
            raise ValueError(f"{what} needs a built lattice and vd >= 1, got vd = {vd}")
        if work is None:
            work = torch.empty(need, dtype=dtype, device=self.device)
        elif work.numel() < need or not work.is_contiguous() or work.dtype != dtype:
            raise ValueError(f"work must be a contiguous {str(dtype).split('.')[-1]} buffer of at least {need} elements")
        res = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            rc = getattr(nv.lib(), symbol)(self._h, ctypes.c_void_p(values.data_ptr()), ctypes.c_void_p(work.data_ptr()), vd,
                                           ctypes.byref(res), _stream_ptr(self.device))
        nv.check(rc, symbol)
        if res.value == values.data_ptr():
            return values[:self.m]
        off = (res.value - work.data_ptr()) // work.element_size()
        return work.view(-1)[off:off + self.m * stride].view(self.m, stride)

    def _apply_variant(self, dtype, symbol, refuse, src, out):
        """The body of apply_t / apply_sym (float64) and apply_t_f32 / apply_sym_f32 (float32): `symbol` is the library's
        call for `dtype`, `refuse` the public method's refusal of the other dtype (fp32 refuses a float64 `out` up front;
        float64 names the dtype of a wrong `out` after the checks of src)."""
        f64 = dtype == torch.float64
        refuse(src, "src")
        if not f64:
            refuse(out, "out")
        _check_f32_cuda(src, "src", f64_ok=f64)
        src = self._src(src, self.n_owned, f64_ok=f64)
        vd = src.shape[1]
        if out is None:
            out = torch.empty((self.n_owned, vd), dtype=dtype, device=self.device)
        elif not f64:
            _check_f32_cuda(out, "out")
        elif out.dtype != torch.float64:
            raise TypeError(f"out must be torch.float64 like src, got {out.dtype}")
        with torch.cuda.device(self.device):
            rc = getattr(nv.lib(), symbol)(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                                           _stream_ptr(self.device))
        nv.check(rc, symbol)
        return out

    def apply_t(self, src, out=None):
        """out = K^T src: slice(blur_t(splat(src))) on the float64 workspace (plx_apply_t_f64).  float64 only."""
        return self._apply_variant(torch.float64, "plx_apply_t_f64", lambda t, name: self._f64_only(t, name, "apply_t"), src, out)

    def apply_sym(self, src, out=None):
        """out = K_s src with K_s = (K + K^T) / 2: slice(blur_sym(splat(src))) (plx_apply_sym_f64).  float64 only.  K_s is
        symmetric to rounding; it is not proven positive."""
        return self._apply_variant(torch.float64, "plx_apply_sym_f64", lambda t, name: self._f64_only(t, name, "apply_sym"),
                                   src, out)

    def sym_f64_kernels(self):
        """Kernels launched by the last transposed or symmetrised float64 call: {"splat": [...], "blur": [...],
        "slice": [...]}; f64_kernels() goes on naming the plain float64 stages."""
        return self._last_kernels("plx_last_sym_f64_kernels", 256)

    # -- the transposed and symmetrised fp32 products (plx_blur_t / plx_blur_sym / plx_apply_t / plx_apply_sym) ------
    # The same two operators in the precision of apply(), under names of their own (the float32 TypeErrors of the methods
    # above stay).  They run one kernel family whatever the shape -- blur_axis_kernel for K^T, blur_dual_kernel for K_s --
    # and follow set_lattice_row_order() as apply() does.
    @staticmethod
    def _f32_only(t, name, what, f64_name):
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise TypeError(f"{what} takes float32 only, got {name} of torch.float64: the float64 form is {f64_name}")

    def blur_t_f32(self, values, scratch=None, vd=None):
        """The adjoint of the fp32 blur(): axes d .. 0, mirrored taps, the general kernel family (plx_blur_t).  Returns the
        tensor that holds the result (either `values` or `scratch`), as blur() does."""
        return self._blur_t(torch.float32, "plx_blur_t", lambda t, name: self._f32_only(t, name, "blur_t_f32", "blur_t"),
                            "float32 buffer", values, scratch, vd)

    def blur_sym_f32(self, values, work=None, vd=None):
        """0.5 * (blur(values) + blur_t_f32(values)) with the general family's bits, in d + 1 launches that advance both
        chains (plx_blur_sym).  `values` [m, values_stride(vd)] float32 is clobbered; `work`: a contiguous float32 buffer
        of at least plx_blur_sym_work_floats elements (allocated when None).  Returns an [m, stride] tensor that views
        `values` or `work`, wherever the result lies."""
        return self._blur_sym(torch.float32, "plx_blur_sym", "plx_blur_sym_work_floats", "blur_sym_f32",
                              lambda t, name: self._f32_only(t, name, "blur_sym_f32", "blur_sym"), values, work, vd)

    def apply_t_f32(self, src, out=None):
        """out = K^T src in float32: slice(blur_t_f32(splat(src))) on the workspace of apply() (plx_apply_t)."""
        return self._apply_variant(torch.float32, "plx_apply_t", lambda t, name: self._f32_only(t, name, "apply_t_f32", "apply_t"),
                                   src, out)

    def apply_sym_f32(self, src, out=None):
        """out = K_s src in float32 with K_s = (K + K^T) / 2: slice(blur_sym_f32(splat(src))) (plx_apply_sym).  K_s is
        symmetric to rounding; it is not proven positive."""
        return self._apply_variant(torch.float32, "plx_apply_sym",
                                   lambda t, name: self._f32_only(t, name, "apply_sym_f32", "apply_sym"), src, out)

    def apply_affine_sym_f32(self, src, scale_shift, out=None, want_dot=False):
        """out = a * K_s src + b * src in float32 (plx_apply_affine_sym): apply_affine() with K_s for K -- the same
        scale_shift, the same want_dot forms (True: (out, dots), 2..256 columns; "partial": (out, work, tiles) with the
        per-tile partial sums left in the lattice's own buffer for the fused CG step)."""
        self._f32_only(src, "src", "apply_affine_sym_f32", "apply_affine(symmetric=True)")
        self._f32_only(scale_shift, "scale_shift", "apply_affine_sym_f32", "apply_affine(symmetric=True)")
        _check_f32_cuda(src, "src")
        src = self._src(src, self.n_owned)
        _check_f32_cuda(scale_shift, "scale_shift", ndim=1)
        assert scale_shift.numel() == 2 and scale_shift.is_contiguous()
        vd = src.shape[1]
        if out is None:
            out = torch.empty((self.n_owned, vd), dtype=torch.float32, device=self.device)
        else:
            _check_f32_cuda(out, "out")
        L = nv.lib()
        dot = work = None
        if want_dot:
            need = int(L.plx_affine_dot_work_floats(self._h, vd))
            if need < 0:
                raise ValueError(f"apply_affine_sym_f32(want_dot=True) needs 2..256 columns on a built lattice, got {vd}")
            if self._dot_work is None or self._dot_work.numel() < need:
                self._dot_work = torch.empty(need, dtype=torch.float32, device=self.device)
            work = self._dot_work
            if want_dot != "partial":
                dot = torch.empty(self.values_stride(vd), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = L.plx_apply_affine_sym(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                                        ctypes.c_void_p(scale_shift.data_ptr()),
                                        ctypes.c_void_p(dot.data_ptr()) if dot is not None else None,
                                        ctypes.c_void_p(work.data_ptr()) if work is not None else None,
                                        _stream_ptr(self.device))
        nv.check(rc, "plx_apply_affine_sym")
        if want_dot == "partial":
            return out, work, int(L.plx_affine_dot_tiles(self._h, vd))
        return (out, dot[:vd]) if want_dot else out

    def sym_kernels_f32(self):
        """Kernels launched by the last transposed or symmetrised fp32 call: {"splat": [...], "blur": [...],
        "slice": [...]}; stage_kernels() goes on naming the plain fp32 stages."""
        return self._last_kernels("plx_last_sym_kernels", 512)

    # -- the true diagonal (plx_diag / plx_diag_f64) ---------------------------
    def diag(self, dtype=torch.float32, rows=None, lattice_rows=False, out=None):
        """K_ii of K = S B_d ... B_0 S^T / (1 + 2^-d) with this build's taps, per point -- what the product computes, not
        the unit diagonal the kernel classes declare; also the diagonal of K^T and of K_s.  Every sum is carried in `dtype`
        (torch.float32: plx_diag, torch.float64: plx_diag_f64).  rows = (begin, count): the caller rows of that range only
        (on a stacked lattice [xout; xin] the range of xin is diag K(x*, x*)).  lattice_rows: the values in lattice position
        order, the whole range only; the call ignores set_lattice_row_order.  One launch, no workspace: graph-capturable."""
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"diag: dtype is torch.float32 or torch.float64, got {dtype}")
        fn = "plx_diag" if dtype == torch.float32 else "plx_diag_f64"
        if not nv.has_symbols(fn):
            raise RuntimeError(f"diag: this libplx.so does not export {fn}: rebuild it (make -C simplex_gp_amd/csrc)")
        begin, count = (0, self.n) if rows is None else self._rows(*rows)
        if lattice_rows and (begin, count) != (0, self.n):
            raise ValueError(f"diag(lattice_rows=True) serves the whole range [0, {self.n}) only")
        if out is None:
            out = torch.empty(count, dtype=dtype, device=self.device)
        else:
            assert out.is_cuda and out.dtype == dtype and out.is_contiguous() and out.numel() == count, \
                f"out must be a contiguous {dtype} CUDA tensor of {count} elements"
        with torch.cuda.device(self.device):
            rc = getattr(nv.lib(), fn)(self._h, begin, count, 1 if lattice_rows else 0, ctypes.c_void_p(out.data_ptr()),
                                       _stream_ptr(self.device))
        nv.check(rc, fn)
        return out

    # -- queries at points that are not the build's (plx_locate / plx_slice_at) ---
    # The operator is K_q(x*, X) = S* B_d ... B_0 S_X^T / (1 + 2^-d): S* holds a query's barycentric weights on those of its
    # d + 1 corners that are vertices of X's lattice, an absent corner contributes nothing.  It is NOT the stacked operator of
    # apply_rows on [x*; X], whose blur also runs through vertices that only the query points create; LatticeQuery.mass says
    # how much of every query this lattice supports.
    @staticmethod
    def _need_query_symbols(who, *names):
        for name in names:
            if not nv.has_symbols(name):
                raise RuntimeError(f"{who}: this libplx.so does not export {name}: rebuild it (make -C simplex_gp_amd/csrc)")

    def locate(self, x, want_mass=True):
        """The corners of the points x [nq, d] (CUDA float32, in the units of the build's positions: already divided by the
        lengthscale; float64 is rounded to float32 as the build does) in this build's vertex numbering: a LatticeQuery.  One
        launch, no workspace: graph-capturable.  Points outside the key range (or NaN / Inf) find nothing: mass 0."""
        self._need_query_symbols("locate", "plx_locate")
        x = _positions_f32(x, "x")
        if x.shape[1] != self.d or x.shape[0] < 1:
            raise ValueError(f"x must be [nq >= 1, {self.d}], got shape {tuple(x.shape)}")
        if x.device != self.device:
            raise ValueError(f"x is on {x.device}, the lattice on {self.device}")
        x = x.contiguous()
        nq, d1 = x.shape[0], self.d + 1
        vid = torch.empty((d1, nq), dtype=torch.int32, device=self.device)
        weight = torch.empty((d1, nq), dtype=torch.float32, device=self.device)
        mass = torch.empty(nq, dtype=torch.float32, device=self.device) if want_mass else None
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_locate(self._h, ctypes.c_void_p(x.data_ptr()), nq, ctypes.c_void_p(vid.data_ptr()),
                                     ctypes.c_void_p(weight.data_ptr()),
                                     ctypes.c_void_p(mass.data_ptr()) if want_mass else None, _stream_ptr(self.device))
        nv.check(rc, "plx_locate")
        return LatticeQuery(vid, weight, mass, nq, self.build_id, x)

    def _check_sliced(self, who, values, query, vd, symbols):
        """What slice_at and the calls of its position gradient check about (values, query, vd) before any device work:
        (f64, vd).  symbols: the library calls `who` needs, (for float32 values, for float64 values)."""
        if not isinstance(query, LatticeQuery):
            raise TypeError(f"query must be a LatticeQuery (Lattice.locate), got {type(query).__name__}")
        _check_f32_cuda(values, "values", f64_ok=True)
        f64 = values.dtype == torch.float64
        self._need_query_symbols(who, *symbols[1 if f64 else 0])
        if query.build_id != self.build_id:
            raise RuntimeError(f"{who}: the lattice was rebuilt since this query was located (build {query.build_id}, now "
                               f"{self.build_id}): locate the points again")
        vd = values.shape[1] if vd is None else int(vd)
        if vd < 1 or values.shape[1] != self.values_stride(vd, values.dtype) or not values.is_contiguous():
            raise ValueError(f"values must be contiguous [m, {self.values_stride(max(vd, 1), values.dtype)}] for vd = {vd}, "
                             f"got shape {tuple(values.shape)}")
        if values.shape[0] < self.m:
            raise ValueError(f"values has {values.shape[0]} rows, the lattice {self.m} vertices")
        if values.device != self.device or query.vid.device != self.device:
            raise ValueError(f"values and query must be on {self.device}")
        return f64, vd

    def slice_at(self, values, query, out=None, vd=None):
        """out[nq, vd] = S* values / (1 + 2^-d) at the located `query`, in the dtype of `values` (a vertex array
        [>= m, values_stride(vd, dtype)], e.g. what blurred() returns).  A query located before the lattice's last build is
        refused: its vertex ids belong to another numbering."""
        f64, vd = self._check_sliced("slice_at", values, query, vd, (("plx_slice_at",), ("plx_slice_at_f64",)))
        fn = "plx_slice_at_f64" if f64 else "plx_slice_at"
        if out is None:
            out = torch.empty((query.nq, vd), dtype=values.dtype, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != values.dtype:
            raise TypeError(f"out must be a {values.dtype} tensor like values")
        elif out.shape != (query.nq, vd) or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be contiguous [{query.nq}, {vd}] on {self.device}")
        with torch.cuda.device(self.device):
            rc = getattr(nv.lib(), fn)(self._h, ctypes.c_void_p(values.data_ptr()), vd, ctypes.c_void_p(query.vid.data_ptr()),
                                       ctypes.c_void_p(query.weight.data_ptr()), query.nq, ctypes.c_void_p(out.data_ptr()),
                                       _stream_ptr(self.device))
        nv.check(rc, fn)
        return out

    def blurred(self, src):
        """(values, vd): splat + blur of src [n, vd] in its dtype, `values` being whichever buffer holds the result -- what
        slice_at() reads.  It does not depend on any query: compute it once, slice it anywhere."""
        values = self.splat(src)
        return self.blur(values, vd=src.shape[1]), src.shape[1]

    def apply_at(self, src, query):
        """K_q(x*, X) src at the located query: slice_at(blurred(src), query)."""
        values, vd = self.blurred(src)
        return self.slice_at(values, query, vd=vd)

    def query_kernels(self):
        """Kernels launched by the last locate / slice_at on this lattice: {"locate": [...], "slice_at": [...]}."""
        self._need_query_symbols("query_kernels", "plx_last_query_kernels")
        names = self._last_kernels("plx_last_query_kernels", 256)
        return {k: names[k] for k in ("locate", "slice_at")}

    # -- the rectangular product: splat / slice by row range (plx_*_rows) ------
    def _rows(self, begin, count):
        begin, count = int(begin), int(count)
        if count < 1 or begin < 0 or begin + count > self.n:
            raise ValueError(f"rows [{begin}, {begin + count}) are not a non-empty range inside [0, {self.n})")
        return begin, count

    def splat_rows(self, src, row_begin, values=None):
        """values = S^T restricted to the caller's rows [row_begin, row_begin + len(src)); every vertex row is written.  In the
        dtype of `src` (float64: plx_splat_rows_f64, over the same range tables)."""
        _check_f32_cuda(src, "src", f64_ok=True)
        src = src.contiguous()
        begin, count = self._rows(row_begin, src.shape[0])
        vd = src.shape[1]
        f64 = src.dtype == torch.float64
        if values is None:
            values = self.new_values(vd, src.dtype)
        elif values.dtype != src.dtype:
            raise TypeError(f"values must be {src.dtype} like src, got {values.dtype}")
        assert values.shape == (self.m, self.values_stride(vd, src.dtype)) and values.is_contiguous()
        fn, name = (nv.lib().plx_splat_rows_f64, "plx_splat_rows_f64") if f64 else (nv.lib().plx_splat_rows, "plx_splat_rows")
        with torch.cuda.device(self.device):
            rc = fn(self._h, ctypes.c_void_p(src.data_ptr()), begin, count, vd, ctypes.c_void_p(values.data_ptr()),
                    _stream_ptr(self.device))
        nv.check(rc, name)
        return values

    def slice_rows(self, values, row_begin, row_count, out=None, vd=None):
        """out[row_count, vd] = rows [row_begin, row_begin + row_count) of S values / (1 + 2^-d), in the dtype of `values`."""
        _check_f32_cuda(values, "values", f64_ok=True)
        vd = values.shape[1] if vd is None else vd
        assert values.shape[1] == self.values_stride(vd, values.dtype) and values.is_contiguous()
        begin, count = self._rows(row_begin, row_count)
        if out is None:
            out = torch.empty((count, vd), dtype=values.dtype, device=self.device)
        elif out.dtype != values.dtype:
            raise TypeError(f"out must be {values.dtype} like values, got {out.dtype}")
        assert out.shape == (count, vd) and out.is_contiguous()
        f64 = values.dtype == torch.float64
        fn, name = (nv.lib().plx_slice_rows_f64, "plx_slice_rows_f64") if f64 else (nv.lib().plx_slice_rows, "plx_slice_rows")
        with torch.cuda.device(self.device):
            rc = fn(self._h, ctypes.c_void_p(values.data_ptr()), vd, begin, count, ctypes.c_void_p(out.data_ptr()),
                    _stream_ptr(self.device))
        nv.check(rc, name)
        return out

    def apply_rows(self, src, src_begin, out_begin, out_count, out=None):
        """out[out_count, vd] = K[out rows, src rows] src: rows [out_begin, out_begin + out_count) of apply() of the
        n-row matrix that holds `src` in rows [src_begin, src_begin + len(src)) and zeros elsewhere (plx_apply_rows; float64:
        plx_apply_rows_f64, equal as values to those rows of the float64 apply()).
        Rows are in the caller's order whatever set_lattice_row_order() says."""
        _check_f32_cuda(src, "src", f64_ok=True)
        src = src.contiguous()
        sb, sc = self._rows(src_begin, src.shape[0])
        ob, oc = self._rows(out_begin, out_count)
        vd = src.shape[1]
        if out is None:
            out = torch.empty((oc, vd), dtype=src.dtype, device=self.device)
        elif out.dtype != src.dtype:
            raise TypeError(f"out must be {src.dtype} like src, got {out.dtype}")
        assert out.shape == (oc, vd) and out.is_contiguous()
        f64 = src.dtype == torch.float64
        fn, name = (nv.lib().plx_apply_rows_f64, "plx_apply_rows_f64") if f64 else (nv.lib().plx_apply_rows, "plx_apply_rows")
        with torch.cuda.device(self.device):
            rc = fn(self._h, ctypes.c_void_p(src.data_ptr()), sb, sc, vd, ctypes.c_void_p(out.data_ptr()), ob, oc,
                    _stream_ptr(self.device))
        nv.check(rc, name)
        return out

    def rows_kernels(self):
        """Kernels launched by the last float32 splat_rows / slice_rows (or apply_rows) on this lattice: {"splat": [...],
        "slice": [...]}; the blur of apply_rows reports through stage_kernels().  apply_backward_rows_f32 reports here too:
        rows_backward_splat_{chunk,wide}_kernel under "splat", rows_backward_contract_{chunk,wide}_kernel under "slice"."""
        return self._last_kernels("plx_last_rows_kernels", 256)

    def rows_f64_kernels(self):
        """... and by the last float64 ones; the blur of a float64 apply_rows reports through f64_kernels()."""
        return self._last_kernels("plx_last_rows_f64_kernels", 256)

    def accepts_rows(self):
        """True when the rows calls serve this lattice: a plain single-shard build without the "reference_growth" replay."""
        if self.n_owned != self.n or self._merged:
            return False
        return not self.reference_growth_info()["replayed"]

    def apply_affine(self, src, scale_shift, out=None, want_dot=False, symmetric=False):
        """out = a * K src + b * src with (a, b) = scale_shift (a 2-element tensor on the device, of the dtype of `src`, read
        there: no host synchronisation on hyper-parameters).  float64: plx_apply_affine_f64, rows always in the caller's
        order, want_dot=True for up to 128 columns, no want_dot="partial"; a mixed pair is a TypeError.  want_dot: also return the column-wise <src, out>
        (the p^T A p of a CG iteration), formed inside the slice kernel; needs 2..256 columns.  want_dot="partial":
        return (out, work, tiles) with the per-tile partial sums of those dots left un-reduced in `work` (the fused CG
        step adds them up itself); `work` is the lattice's own buffer, valid until the next such call.
        symmetric=True (float64 only): K_s = (K + K^T) / 2 for K (plx_apply_affine_sym_f64), everything else unchanged."""
        if symmetric:
            self._f64_only(src, "src", "apply_affine(symmetric=True)")
        if isinstance(src, torch.Tensor) and isinstance(scale_shift, torch.Tensor) and src.dtype != scale_shift.dtype:
            raise TypeError(f"src and scale_shift must both be float32 or both float64, got {src.dtype} and "
                            f"{scale_shift.dtype}")
        if isinstance(src, torch.Tensor) and src.dtype == torch.float64:
            return self._apply_affine_f64(src, scale_shift, out, want_dot, symmetric)
        src = self._src(src, self.n_owned)
        _check_f32_cuda(scale_shift, "scale_shift", ndim=1)
        assert scale_shift.numel() == 2 and scale_shift.is_contiguous()
        vd = src.shape[1]
        if out is None:
            out = torch.empty((self.n_owned, vd), dtype=torch.float32, device=self.device)
        if want_dot:
            L = nv.lib()
            need = int(L.plx_affine_dot_work_floats(self._h, vd))
            if need < 0:
                raise ValueError(f"apply_affine(want_dot=True) needs 2..256 columns on a built lattice, got {vd}")
            if self._dot_work is None or self._dot_work.numel() < need:
                self._dot_work = torch.empty(need, dtype=torch.float32, device=self.device)
            if want_dot == "partial":
                # the slice kernel's per-tile partial sums stay in the work buffer: (out, partials, tiles) for
                # plx_cg_step_update_fused, which adds them up itself (no stand-alone reduction launch)
                with torch.cuda.device(self.device):
                    rc = L.plx_apply_affine_dot(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                                                ctypes.c_void_p(scale_shift.data_ptr()), None,
                                                ctypes.c_void_p(self._dot_work.data_ptr()), _stream_ptr(self.device))
                nv.check(rc, "plx_apply_affine_dot")
                return out, self._dot_work, int(L.plx_affine_dot_tiles(self._h, vd))
            dot = torch.empty(self.values_stride(vd), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                rc = L.plx_apply_affine_dot(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(scale_shift.data_ptr()), ctypes.c_void_p(dot.data_ptr()),
                                            ctypes.c_void_p(self._dot_work.data_ptr()), _stream_ptr(self.device))
            nv.check(rc, "plx_apply_affine_dot")
            return out, dot[:vd]
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_apply_affine(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_void_p(scale_shift.data_ptr()), _stream_ptr(self.device))
        nv.check(rc, "plx_apply_affine")
        return out

    def affine_dot_f64_ok(self, vd):
        """True when the float64 apply_affine(want_dot=True) serves vd columns on this build (plx_affine_dot_work_doubles)."""
        return int(nv.lib().plx_affine_dot_work_doubles(self._h, int(vd))) >= 0

    def _apply_affine_f64(self, src, scale_shift, out, want_dot, symmetric=False):
        """The float64 form of apply_affine (plx_apply_affine_f64; symmetric: plx_apply_affine_sym_f64): rows in the caller's order, scale_shift a float64
        2-vector on the device; want_dot=True for up to 128 columns; there is no fused CG step in double, hence no
        want_dot="partial"."""
        if want_dot == "partial":
            raise ValueError('apply_affine(want_dot="partial") has no float64 form: there is no fused CG step in double')
        src = self._src(src, self.n_owned, f64_ok=True)
        _check_f32_cuda(scale_shift, "scale_shift", ndim=1, f64_ok=True)
        assert scale_shift.numel() == 2 and scale_shift.is_contiguous()
        vd = src.shape[1]
        if out is None:
            out = torch.empty((self.n_owned, vd), dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64:
            raise TypeError(f"out must be torch.float64 like src, got {out.dtype}")
        L = nv.lib()
        dot = work = None
        if want_dot:
            need = int(L.plx_affine_dot_work_doubles(self._h, vd))
            if need < 0:
                raise ValueError(f"apply_affine(want_dot=True) in float64 needs 1..128 columns on a built lattice, got {vd}")
            if self._dot_work64 is None or self._dot_work64.numel() < need:
                self._dot_work64 = torch.empty(need, dtype=torch.float64, device=self.device)
            work = self._dot_work64
            dot = torch.empty(vd, dtype=torch.float64, device=self.device)
        name = "plx_apply_affine_sym_f64" if symmetric else "plx_apply_affine_f64"
        with torch.cuda.device(self.device):
            rc = getattr(L, name)(self._h, ctypes.c_void_p(src.data_ptr()), vd, ctypes.c_void_p(out.data_ptr()),
                                  ctypes.c_void_p(scale_shift.data_ptr()),
                                  ctypes.c_void_p(dot.data_ptr()) if want_dot else None,
                                  ctypes.c_void_p(work.data_ptr()) if want_dot else None, _stream_ptr(self.device))
        nv.check(rc, name)
        return (out, dot) if want_dot else out

    @staticmethod
    def backward_fusable(nrhs, d):
        """True when plx_apply_backward covers this shape: 125..512 columns and 2*nrhs + d <= 62."""
        return 32 <= (2 * nrhs * (1 + d) + 3) // 4 <= 128 and 2 * nrhs + d <= 62

    BACKWARD_F64_MAX_COLUMNS = 2048      # kBackwardF64MaxCols of plx_backward_f64.hip: the contraction's on-chip row

    @staticmethod
    def backward_f64_ok(nrhs, d):
        """True when plx_apply_backward_f64 covers this shape: nrhs >= 1 and 2*nrhs*(1+d) <= 2048 stacked columns."""
        return nrhs >= 1 and d >= 1 and 2 * nrhs * (1 + d) <= Lattice.BACKWARD_F64_MAX_COLUMNS

    def apply_backward(self, grad_out, src, ref, want_grad_src=True):
        """Position gradient of out = K(ref) src for a lattice built on `ref` with the DERIVATIVE taps
        (bilateral_kernel.py:113-123), fused: returns (grad_ref [n, d], grad_src [n, nrhs] or None).  All three float64:
        plx_apply_backward_f64 (the lattice is the one of `ref` rounded to float32, `ref` itself enters the stack and the
        contraction in double; rows always in the caller's order; every shape backward_f64_ok names).  A mixed combination
        is a TypeError."""
        dtypes = {t.dtype for t in (grad_out, src, ref) if isinstance(t, torch.Tensor)}
        if len(dtypes) > 1:
            raise TypeError("grad_out, src and ref must all be float32 or all float64, got "
                            + ", ".join(str(t.dtype) for t in (grad_out, src, ref) if isinstance(t, torch.Tensor)))
        if dtypes == {torch.float64}:
            return self._apply_backward_f64(grad_out, src, ref, want_grad_src)
        g = self._src(grad_out, self.n_owned)
        src = self._src(src, self.n_owned)
        ref = self._src(ref, self.n_owned)
        if g.shape != src.shape or ref.shape[1] != self.d:
            raise ValueError(f"Incompatible shapes {tuple(g.shape)}, {tuple(src.shape)}, {tuple(ref.shape)}")
        grad_ref = torch.empty_like(ref)
        grad_src = torch.empty_like(src) if want_grad_src else None
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_apply_backward(self._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                             ctypes.c_void_p(ref.data_ptr()), src.shape[1],
                                             ctypes.c_void_p(grad_ref.data_ptr()),
                                             ctypes.c_void_p(grad_src.data_ptr()) if want_grad_src else None,
                                             _stream_ptr(self.device))
        nv.check(rc, "plx_apply_backward")
        return grad_ref, grad_src

    def _apply_backward_f64(self, grad_out, src, ref, want_grad_src):
        """The float64 form of apply_backward (plx_apply_backward_f64)."""
        g = self._src(grad_out, self.n_owned, f64_ok=True)
        src = self._src(src, self.n_owned, f64_ok=True)
        ref = self._src(ref, self.n_owned, f64_ok=True)
        if g.shape != src.shape or ref.shape[1] != self.d:
            raise ValueError(f"Incompatible shapes {tuple(g.shape)}, {tuple(src.shape)}, {tuple(ref.shape)}")
        grad_ref = torch.empty_like(ref)
        grad_src = torch.empty_like(src) if want_grad_src else None
        with torch.cuda.device(self.device):
            rc = nv.lib().plx_apply_backward_f64(self._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                                 ctypes.c_void_p(ref.data_ptr()), src.shape[1],
                                                 ctypes.c_void_p(grad_ref.data_ptr()),
                                                 ctypes.c_void_p(grad_src.data_ptr()) if want_grad_src else None,
                                                 _stream_ptr(self.device))
        nv.check(rc, "plx_apply_backward_f64")
        return grad_ref, grad_src

    BACKWARD_ROWS_F64_MAX_STRIDE = 2048      # kBackwardF64MaxCols on the row stride of the half stack

    @staticmethod
    def backward_rows_f64_ok(nrhs, d):
        """True when plx_apply_backward_rows_f64 covers this shape: nrhs >= 1, d >= 1 and the row of the half stack --
        nrhs*(1+d) doubles rounded up to even -- within 2048."""
        return nrhs >= 1 and d >= 1 and (nrhs * (1 + d) + 1) // 2 * 2 <= Lattice.BACKWARD_ROWS_F64_MAX_STRIDE

    def apply_backward_rows(self, a, a_begin, b, b_begin, x, want_filtered=True):
        """One side of the position gradient of the rectangular product, for a lattice built with the DERIVATIVE taps on
        the stacked positions `x` [n, d] rounded to float32 (plx_apply_backward_rows_f64): the half stack [a | a (x) x] of
        rows [a_begin, a_begin + len(a)) is filtered to rows [b_begin, b_begin + len(b)) and contracted there against b.
        Returns (grad_x [len(b), d], filtered [len(b), nrhs] or None); filtered is the derivative-tap filter of `a` on the
        rows of b.  (a = grad_out on the out rows, b = src on the source rows) is the gradient of the source rows'
        positions, (a = src, b = grad_out) that of the out rows'.  float64 CUDA tensors only: there is no fp32 form."""
        return self._apply_backward_rows(torch.float64, "plx_apply_backward_rows_f64", "apply_backward_rows has no fp32 form",
                                         a, a_begin, b, b_begin, x, want_filtered)

    def _apply_backward_rows(self, dtype, symbol, who, a, a_begin, b, b_begin, x, want_filtered):
        """The body of apply_backward_rows (float64) and apply_backward_rows_f32 (float32): `symbol` is the library's call
        for `dtype`, `who` opens the refusal of any other dtype with the public method's name."""
        for t, name in ((a, "a"), (b, "b"), (x, "x")):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor")
        if {a.dtype, b.dtype, x.dtype} != {dtype}:
            raise TypeError(f"{who}: a, b and x must all be {str(dtype).split('.')[-1]}, got "
                            f"{a.dtype}, {b.dtype} and {x.dtype}")
        f64_ok = dtype == torch.float64
        for t, name in ((a, "a"), (b, "b"), (x, "x")):
            _check_f32_cuda(t, name, f64_ok=f64_ok)
        a, b, x = a.contiguous(), b.contiguous(), self._src(x, self.n, f64_ok=f64_ok)
        ab, ac = self._rows(a_begin, a.shape[0])
        bb, bc = self._rows(b_begin, b.shape[0])
        if a.shape[1] != b.shape[1] or x.shape[1] != self.d:
            raise ValueError(f"Incompatible shapes {tuple(a.shape)}, {tuple(b.shape)}, {tuple(x.shape)}")
        nrhs = a.shape[1]
        grad_x = torch.empty((bc, self.d), dtype=dtype, device=self.device)
        filtered = torch.empty((bc, nrhs), dtype=dtype, device=self.device) if want_filtered else None
        with torch.cuda.device(self.device):
            rc = getattr(nv.lib(), symbol)(self._h, ctypes.c_void_p(a.data_ptr()), ab, ac, ctypes.c_void_p(b.data_ptr()), bb, bc,
                                           ctypes.c_void_p(x.data_ptr()), nrhs, ctypes.c_void_p(grad_x.data_ptr()),
                                           ctypes.c_void_p(filtered.data_ptr()) if want_filtered else None,
                                           _stream_ptr(self.device))
        nv.check(rc, symbol)
        return grad_x, filtered

    BACKWARD_ROWS_MAX_STRIDE = 4096          # kBackwardRowsMaxCols on the row stride of the fp32 half stack

    @staticmethod
    def backward_rows_ok(nrhs, d):
        """True when plx_apply_backward_rows covers this shape: nrhs >= 1, d >= 1 and the row of the half stack --
        nrhs*(1+d) floats rounded up to a multiple of 4 -- within 4096."""
        return nrhs >= 1 and d >= 1 and (nrhs * (1 + d) + 3) // 4 * 4 <= Lattice.BACKWARD_ROWS_MAX_STRIDE

    def apply_backward_rows_f32(self, a, a_begin, b, b_begin, x, want_filtered=True):
        """The fp32 form of apply_backward_rows (plx_apply_backward_rows), with its return convention: the lattice is built
        with the DERIVATIVE taps on `x` [n, d].  float32 CUDA tensors only; the name is its own because apply_backward_rows
        refuses every float32 tensor and does not dispatch on dtype."""
        return self._apply_backward_rows(torch.float32, "plx_apply_backward_rows", "apply_backward_rows_f32",
                                         a, a_begin, b, b_begin, x, want_filtered)

    # -- introspection (parity tests) --------------------------------------
    def export(self, which):
        L = nv.lib()
        nbytes = int(L.plx_export_bytes(self._h, which))
        if nbytes < 0:
            raise ValueError(f"unknown array {which}")
        n, m, d, r = self.n, self.m, self.d, self.order
        dtype, shape = {
            nv.ARRAY_KEYS: (np.int16, (m, d)),
            nv.ARRAY_ENTRY_VERTEX: (np.int32, (d + 1, n)),
            nv.ARRAY_ENTRY_WEIGHT: (np.float32, (d + 1, n)),
            nv.ARRAY_NEIGHBORS: (np.int32, (d + 1, 2 * r, m)),
            nv.ARRAY_ROW_PTR: (np.int32, (m + 1,)),
            nv.ARRAY_CSR_POINT: (np.int32, (self.n_owned * (d + 1),)),
            nv.ARRAY_CSR_WEIGHT: (np.float32, (self.n_owned * (d + 1),)),
            nv.ARRAY_POINT_PERM: (np.uint32, (n,)),
        }[which]
        out = np.empty(shape, dtype)
        assert out.nbytes == nbytes, (out.nbytes, nbytes)
        with torch.cuda.device(self.device):
            rc = L.plx_export(self._h, which, out.ctypes.data_as(ctypes.c_void_p), nbytes,
                              _stream_ptr(self.device))
        nv.check(rc, "plx_export")
        return out


_scratch = {}


def _scratch_lattice(device):
    key = device.index
    lat = _scratch.get(key)
    if lat is None:
        lat = _scratch[key] = Lattice(device)
    return lat


def filter(src, ref, coeffs):
    """filter(src[N,vd], ref[N,d], coeffs[R]) -> out[N,vd]   (reference boundary).

    Builds a fresh lattice for `ref` on every call, exactly like the reference
    (permutohedral.h:272); only the device buffers are recycled between calls.

    src and ref BOTH float64 (the reference's GPU path dispatches double too): the lattice is built on the positions
    rounded to float32 and the product runs in double on it (Lattice.apply).  A mixed pair is a TypeError.
    """
    both = isinstance(src, torch.Tensor) and isinstance(ref, torch.Tensor)
    if both and src.dtype != ref.dtype:
        raise TypeError(f"src and ref must both be float32 or both float64, got {src.dtype} and {ref.dtype}")
    both_f64 = both and src.dtype == torch.float64
    _check_f32_cuda(src, "src", f64_ok=both_f64)
    _check_f32_cuda(ref, "ref", f64_ok=both_f64)
    if src.shape[0] != ref.shape[0]:
        raise ValueError("Incompatible shapes {}, and {}".format(tuple(src.shape), tuple(ref.shape)))
    if src.device != ref.device:
        raise ValueError("src and ref must be on the same device")
    if both_f64:
        return _scratch_lattice(src.device).build(_positions_f32(ref), coeffs).apply(src)
    return _scratch_lattice(src.device).filter_once(src, ref, coeffs)
