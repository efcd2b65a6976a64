"""The splat at query points: S*^T g, the adjoint of Lattice.slice_at, and with it K_q^T g = K(X, x*) g.

    splat_at(g, query)[v] = sum over (q, r) with vid[r, q] == v of w[r, q] * g[q]

Two steps, no atomics: a QueryPlan, built once per located query (its found corners sorted by vertex with the build's stable
sort: plx_query_plan), then one launch of the row-range splat's kernels per call (plx_splat_at / plx_splat_at_f64).  Inside
a vertex the corners are summed in ascending pair index r * nq + q, so two plans of one query give the same bits.
slice_at_adjoint divides by 1 + 2^-d and is the gradient of <grad_out, slice_at(values, query)> with respect to `values`;
apply_at_t adds the transposed blur and the build's slice.  DESIGN.md section 28.

Functions of a built Lattice, not methods of it: tests/test_interleave.py holds every launching method of the Lattice class
to an op of the interleave table, and these calls are not in that table yet.
"""
import ctypes

import torch

from . import _native as nv
from .lattice import LatticeQuery, _check_f32_cuda, _stream_ptr

_PLAN_SYMBOLS = ("plx_query_plan_bytes", "plx_query_plan")


class QueryPlan:
    """The corners of a located query sorted by vertex (plan()): `buffer` (uint8, the tables and the sort's scratch, laid out
    by the library), for `nq` queries on build `build_id` of the lattice.  The library cannot tell a plan of another build
    or another nq from the right one; splat_at compares both and refuses."""
    __slots__ = ("buffer", "nq", "build_id")

    def __init__(self, buffer, nq, build_id):
        self.buffer, self.nq, self.build_id = buffer, int(nq), int(build_id)


def _check_query(lat, who, query):
    if not isinstance(query, LatticeQuery):
        raise TypeError(f"query must be a LatticeQuery (Lattice.locate), got {type(query).__name__}")
    if query.build_id != lat.build_id:
        raise RuntimeError(f"{who}: the lattice was rebuilt since this query was located (build {query.build_id}, now "
                           f"{lat.build_id}): locate the points again")
    if query.vid.device != lat.device:
        raise ValueError(f"query must be on {lat.device}")


def plan(lat, query):
    """The QueryPlan of a located query: one key kernel, the stable sort, one table kernel, one row-pointer kernel.  Launches
    only (the buffer is allocated here, by torch)."""
    lat._need_query_symbols("query_adjoint.plan", *_PLAN_SYMBOLS)
    _check_query(lat, "query_adjoint.plan", query)
    nbytes = int(nv.lib().plx_query_plan_bytes(lat._h, query.nq))
    if nbytes < 0:
        raise ValueError(f"query_adjoint.plan: no plan for nq = {query.nq} on this lattice (unbuilt, or nq (d + 1) past the "
                         "sort's limit)")
    buffer = torch.empty(nbytes, dtype=torch.uint8, device=lat.device)
    with torch.cuda.device(lat.device):
        rc = nv.lib().plx_query_plan(lat._h, ctypes.c_void_p(query.vid.data_ptr()), ctypes.c_void_p(query.weight.data_ptr()),
                                     query.nq, ctypes.c_void_p(buffer.data_ptr()), _stream_ptr(lat.device))
    nv.check(rc, "plx_query_plan")
    return QueryPlan(buffer, query.nq, lat.build_id)


_make_plan = plan      # the calls below take a `plan` argument of their own


def _check_plan(lat, who, query, plan_):
    if not isinstance(plan_, QueryPlan):
        raise TypeError(f"plan must be a QueryPlan (query_adjoint.plan), got {type(plan_).__name__}")
    if plan_.build_id != lat.build_id or plan_.nq != query.nq:
        raise RuntimeError(f"{who}: the lattice was rebuilt since this plan was made, or it is the plan of another query "
                           f"(plan: build {plan_.build_id}, nq {plan_.nq}; now build {lat.build_id}, nq {query.nq}): "
                           "plan the query again")


def splat_at(lat, grad_out, query, plan=None, values=None):
    """values [m, values_stride(vd, dtype)] = S*^T grad_out in the dtype of grad_out [nq, vd] (float32 or float64): every
    row written, exact zeros where no corner of the query lands and in the stride padding.  A missing plan is built."""
    _check_f32_cuda(grad_out, "grad_out", f64_ok=True)
    f64 = grad_out.dtype == torch.float64
    fn = "plx_splat_at_f64" if f64 else "plx_splat_at"
    lat._need_query_symbols("splat_at", fn, *(() if plan is not None else _PLAN_SYMBOLS))
    _check_query(lat, "splat_at", query)
    vd = grad_out.shape[1]
    if grad_out.shape[0] != query.nq or vd < 1 or grad_out.device != lat.device:
        raise ValueError(f"grad_out must be [{query.nq}, vd >= 1] on {lat.device}, got shape {tuple(grad_out.shape)} on "
                         f"{grad_out.device}")
    if plan is None:
        plan = _make_plan(lat, query)
    _check_plan(lat, "splat_at", query, plan)
    grad_out = grad_out.contiguous()
    shape = (lat.m, lat.values_stride(vd, grad_out.dtype))
    if values is None:
        values = torch.empty(shape, dtype=grad_out.dtype, device=lat.device)
    elif not isinstance(values, torch.Tensor) or values.dtype != grad_out.dtype:
        raise TypeError(f"values must be a {grad_out.dtype} tensor like grad_out")
    elif tuple(values.shape) != shape or not values.is_contiguous() or values.device != lat.device:
        raise ValueError(f"values must be contiguous [{shape[0]}, {shape[1]}] on {lat.device}, got shape {tuple(values.shape)}")
    with torch.cuda.device(lat.device):
        rc = getattr(nv.lib(), fn)(lat._h, ctypes.c_void_p(plan.buffer.data_ptr()), ctypes.c_void_p(grad_out.data_ptr()), vd,
                                   query.nq, ctypes.c_void_p(values.data_ptr()), _stream_ptr(lat.device))
    nv.check(rc, fn)
    return values


def slice_at_adjoint(lat, grad_out, query, plan=None):
    """The gradient of <grad_out, lat.slice_at(values, query)> with respect to `values`, [m, values_stride(vd, dtype)]:
    splat_at(grad_out / (1 + 2^-d)), the denominator in the dtype's own arithmetic."""
    _check_f32_cuda(grad_out, "grad_out", f64_ok=True)
    lat._need_query_symbols("slice_at_adjoint", "plx_splat_at_f64" if grad_out.dtype == torch.float64 else "plx_splat_at")
    denom = torch.tensor(1.0 + 2.0 ** -lat.d, dtype=grad_out.dtype, device=grad_out.device)
    return splat_at(lat, grad_out / denom, query, plan=plan)


def apply_at_t(lat, grad_out, query, plan=None, out=None):
    """K_q^T grad_out = K(X, x*) grad_out, [n, vd] in the dtype of grad_out: lat.slice(blur_t(splat_at(grad_out))), with
    blur_t for float64 and blur_t_f32 for float32.  Rows as slice() gives them: float32 in the order set_lattice_row_order()
    says, float64 always in the caller's."""
    values = splat_at(lat, grad_out, query, plan=plan)
    vd = grad_out.shape[1]
    blur_t = lat.blur_t if grad_out.dtype == torch.float64 else lat.blur_t_f32
    return lat.slice(blur_t(values, vd=vd), out=out, vd=vd)


def kernels(lat):
    """Kernels launched by the last plan / splat_at on `lat`: {"plan": [...], "splat_at": [...]}."""
    lat._need_query_symbols("query_adjoint.kernels", "plx_last_splat_at_kernels")
    names = lat._last_kernels("plx_last_splat_at_kernels", 256)
    return {k: names.get(k, []) for k in ("plan", "splat_at")}
