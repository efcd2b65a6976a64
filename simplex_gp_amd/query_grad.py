"""The position gradient of a query: d <grad_out, Lattice.slice_at(values, Lattice.locate(x))> / d x.

slice_at is linear in the weights and, inside the simplex locate chose, the weights are affine in x: the exact derivative of
what the forward computes is the corner dots t[r, q] = <grad_out[q], values[vid[r, q]]> / (1 + 2^-d) (plx_slice_at_dots)
pulled back through the embedding (plx_locate_pullback).  Two launches, no atomics, no workspace; `values` gets no gradient.
DESIGN.md section 27.

Functions of a built Lattice, not methods of it: tests/test_interleave.py holds every launching method of the Lattice class
to an op of the interleave table, and these calls are not in that table yet.
"""
import ctypes

import torch

from . import _native as nv
from .lattice import LatticeQuery, _check_f32_cuda, _stream_ptr


def _symbols(f64):
    return ("plx_slice_at_dots_f64", "plx_locate_pullback_f64") if f64 else ("plx_slice_at_dots", "plx_locate_pullback")


def slice_at_dots(lat, values, query, grad_out, vd=None):
    """t [d+1, nq] in values.dtype: t[r, q] = <grad_out[q], values[vid[r, q]]> / (1 + 2^-d), exactly 0 where the corner is
    absent -- the derivative of <grad_out, lat.slice_at(values, query)> with respect to the weights.  grad_out [nq, vd] in
    the dtype of `values`.  The checks of Lattice.slice_at; one launch."""
    f64, vd = lat._check_sliced("slice_at_dots", values, query, vd, (_symbols(False)[:1], _symbols(True)[:1]))
    if not isinstance(grad_out, torch.Tensor) or grad_out.dtype != values.dtype:
        raise TypeError(f"grad_out must be a {values.dtype} tensor like values")
    if grad_out.shape != (query.nq, vd) or grad_out.device != lat.device:
        raise ValueError(f"grad_out must be [{query.nq}, {vd}] on {lat.device}, got shape {tuple(grad_out.shape)}")
    grad_out = grad_out.contiguous()
    t = torch.empty((lat.d + 1, query.nq), dtype=values.dtype, device=lat.device)
    fn = _symbols(f64)[0]
    with torch.cuda.device(lat.device):
        rc = getattr(nv.lib(), fn)(lat._h, ctypes.c_void_p(values.data_ptr()), vd, ctypes.c_void_p(query.vid.data_ptr()),
                                   ctypes.c_void_p(grad_out.data_ptr()), query.nq, ctypes.c_void_p(t.data_ptr()),
                                   _stream_ptr(lat.device))
    nv.check(rc, fn)
    return t


def locate_pullback(lat, query, t):
    """grad_x [nq, d] in t.dtype from t [d+1, nq], the derivative of a scalar with respect to the weights of `query`: its
    pull-back through the embedding, in the simplex locate chose (recomputed from query.x).  One launch."""
    if not isinstance(query, LatticeQuery):
        raise TypeError(f"query must be a LatticeQuery (Lattice.locate), got {type(query).__name__}")
    _check_f32_cuda(t, "t", f64_ok=True)
    fn = _symbols(t.dtype == torch.float64)[1]
    lat._need_query_symbols("locate_pullback", fn)
    if query.build_id != lat.build_id:
        raise RuntimeError(f"locate_pullback: the lattice was rebuilt since this query was located (build {query.build_id}, "
                           f"now {lat.build_id}): locate the points again")
    if query.x is None:
        raise ValueError("locate_pullback: this LatticeQuery does not carry its positions (x): locate the points again")
    if tuple(query.x.shape) != (query.nq, lat.d) or query.x.dtype != torch.float32 or not query.x.is_contiguous():
        raise ValueError(f"query.x must be contiguous float32 [{query.nq}, {lat.d}]")
    if tuple(t.shape) != (lat.d + 1, query.nq) or not t.is_contiguous():
        raise ValueError(f"t must be contiguous [{lat.d + 1}, {query.nq}], got shape {tuple(t.shape)}")
    if t.device != lat.device or query.x.device != lat.device:
        raise ValueError(f"t and query must be on {lat.device}")
    gx = torch.empty((query.nq, lat.d), dtype=t.dtype, device=lat.device)
    with torch.cuda.device(lat.device):
        rc = getattr(nv.lib(), fn)(lat._h, ctypes.c_void_p(query.x.data_ptr()), ctypes.c_void_p(t.data_ptr()), query.nq,
                                   ctypes.c_void_p(gx.data_ptr()), _stream_ptr(lat.device))
    nv.check(rc, fn)
    return gx


def slice_at_backward(lat, values, query, grad_out, vd=None):
    """grad_x [nq, d] in values.dtype: the gradient of <grad_out, lat.slice_at(values, query)> with respect to the positions
    the query was located at (in the build's units: already divided by the lengthscale) -- slice_at_dots, then
    locate_pullback.  Exact for the piecewise-linear function the forward computes; `values` is a constant here."""
    if isinstance(values, torch.Tensor):
        lat._need_query_symbols("slice_at_backward", *_symbols(values.dtype == torch.float64))
    return locate_pullback(lat, query, slice_at_dots(lat, values, query, grad_out, vd=vd))


def kernels(lat):
    """Kernels launched by the last slice_at_dots / locate_pullback on `lat`: {"dots": [...], "pullback": [...]}."""
    lat._need_query_symbols("query_grad.kernels", "plx_last_query_kernels")
    names = lat._last_kernels("plx_last_query_kernels", 256)
    return {k: names.get(k, []) for k in ("dots", "pullback")}
