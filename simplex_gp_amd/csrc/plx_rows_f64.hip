// plx_rows_f64.hip -- the float64 rectangular product K[out rows, src rows] v: the fp64 splat and slice restricted to a range
// of the caller's rows (plx_splat_rows_f64 / plx_slice_rows_f64 / plx_apply_rows_f64, include/plx.h; the entry points and
// their argument checks are in plx_api.hip).  The blur in the middle is plx_f64.hip's.
//
// The tables are those of plx_rows.hip (RowsRange: ptr / row / w per vertex, pos / prow per point): they hold no values, so
// a range that an fp32 call built serves the fp64 call and the reverse.  The arithmetic is that of plx_f64.hip, formed from
// the same pieces (plx_kernels.h: VecOps<double2>::fma, f64_vertex_sum, f64_point_sum) in the same order: a range's corner
// table is a stable compaction of the vertex-sorted corners, so a vertex row keeps the order of its surviving terms, and a
// term dropped here is fma(w, 0, acc) = acc there.  Hence plx_apply_rows_f64 equals, as values, the wanted rows of
// plx_apply_f64 of the zero-padded right-hand side.
//
// Kernels (256-thread workgroups, wave64; value rows are whole 16-byte chunks of two doubles), gated as in plx_f64.hip:
//   rows64_splat_v1_kernel     vd = 1: one thread per vertex adds up the range's corners there, in order;
//   rows64_splat_chunk_kernel  1..64 chunks per row: a group of G = 2^k >= chunks lanes per vertex, one lane per chunk;
//   rows64_splat_wide_kernel   more than 64 chunks: one wave per vertex, its lanes stride over the chunks;
//   rows64_slice_v1_kernel / rows64_slice_chunk_kernel / rows64_slice_wide_kernel: the same three shapes per entry j of the
//                              range's position table, p = pos[j] in ascending lattice order, stored to out[prow[j]].
// Every vertex row is written by exactly one thread per chunk (zero where the range has no corner there): no atomics, no
// zero-fill pass, bitwise reproducible.

#include "plx_kernels.h"

#include <math.h>

namespace plx {

// ---- splat ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rows64_splat_v1_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                 const float *__restrict__ w, const double *__restrict__ src,
                                                                 int m, double *__restrict__ values)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    double acc = 0.0;
    for (int j = ptr[v], j1 = ptr[v + 1]; j < j1; ++j) acc += (double)w[j] * src[row[j]];
    values[v] = acc;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void rows64_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                    const float *__restrict__ w,
                                                                    const double *__restrict__ src, int vd, int nch,
                                                                    int shift, int m, double2 *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = f64_vertex_sum<VEC>(row, w, ptr[v], ptr[v + 1], src, vd, ch);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void rows64_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                   const float *__restrict__ w,
                                                                   const double *__restrict__ src, int vd, int nch, int m,
                                                                   double2 *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = f64_vertex_sum<VEC>(row, w, j0, j1, src, vd, ch);
}

// ---- slice ---------------------------------------------------------------------------------------------------------
// D1 > 0: d + 1 compiled in (all index loads, then all gathers, then the ordered sum); 0: the run-time form
template <int D1>
__global__ __launch_bounds__(kBlock) void rows64_slice_v1_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                                 const int *__restrict__ evid, const float *__restrict__ ew,
                                                                 int n, int d1, int count, const double *__restrict__ values,
                                                                 double denom, double *__restrict__ out)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    const int p = pos[j];
    double acc = 0.0;
    if constexpr (D1 > 0) {
        int v[D1];
        double g[D1];
#pragma unroll
        for (int r = 0; r < D1; ++r) v[r] = evid[(size_t)r * n + p];
#pragma unroll
        for (int r = 0; r < D1; ++r) g[r] = values[v[r]];
#pragma unroll
        for (int r = 0; r < D1; ++r) acc += (double)ew[(size_t)r * n + p] * g[r];
    } else {
        for (int r = 0; r < d1; ++r) acc += (double)ew[(size_t)r * n + p] * values[evid[(size_t)r * n + p]];
    }
    out[prow[j]] = acc / denom;
}

template <bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void rows64_slice_chunk_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                                    const int *__restrict__ evid,
                                                                    const float *__restrict__ ew, int n, int d1, int count,
                                                                    const double2 *__restrict__ values, int vd, int nch,
                                                                    int shift, double denom, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (j >= count || ch >= nch) return;
    const int p = pos[j];
    double2 acc;
    if constexpr (D1 > 0) {
        int v[D1];
        double2 g[D1];
#pragma unroll
        for (int r = 0; r < D1; ++r) v[r] = evid[(size_t)r * n + p];
#pragma unroll
        for (int r = 0; r < D1; ++r) g[r] = values[(size_t)v[r] * nch + ch];
        acc = VecOps<double2>::zero();
#pragma unroll
        for (int r = 0; r < D1; ++r) VecOps<double2>::fma(acc, (double)ew[(size_t)r * n + p], g[r]);
        acc = make_double2(acc.x / denom, acc.y / denom);
    } else {
        acc = f64_point_sum(evid, ew, n, p, d1, values, nch, ch, denom);
    }
    f64_store_chunk<VEC>(out, (size_t)prow[j], vd, ch, acc);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void rows64_slice_wide_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                                   const int *__restrict__ evid, const float *__restrict__ ew,
                                                                   int n, int d1, int count,
                                                                   const double2 *__restrict__ values, int vd, int nch,
                                                                   double denom, double *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (j >= count) return;
    const int p = pos[j];
    const size_t row = (size_t)prow[j];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        f64_store_chunk<VEC>(out, row, vd, ch, f64_point_sum(evid, ew, n, p, d1, values, nch, ch, denom));
}

// ---- launch side ---------------------------------------------------------------------------------------------------
const char *splat_rows_f64_launch(const int *ptr, const int *row, const float *w, const double *d_src, int vd, int m,
                                  double *d_values, hipStream_t stream)
{
    const int nch = values_stride_f64(vd) / 2;
    const bool vec = f64_vec_ok(d_src, vd);
    double2 *v2 = reinterpret_cast<double2 *>(d_values);
    const char *kn_rows64_splat;          // (named as the member the row-range splat keeps it in)
    if (vd == 1) {
        kn_rows64_splat = "rows64_splat_v1_kernel";
        rows64_splat_v1_kernel<<<ceil_div(m, kBlock), kBlock, 0, stream>>>(ptr, row, w, d_src, m, d_values);
    } else if (nch <= kChunkGroupMax) {
        kn_rows64_splat = "rows64_splat_chunk_kernel";
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        if (vec) rows64_splat_chunk_kernel<true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, v2);
        else rows64_splat_chunk_kernel<false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, v2);
    } else {
        kn_rows64_splat = "rows64_splat_wide_kernel";
        const int grid = ceil_div(m, kBlock / 64);
        if (vec) rows64_splat_wide_kernel<true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, v2);
        else rows64_splat_wide_kernel<false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, v2);
    }
    return kn_rows64_splat;
}

int splat_rows_f64_impl(plx_lattice *L, const double *d_src, int64_t begin, int64_t count, int vd, double *d_values,
                        hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, begin, count);
    PLX_TRY(ensure_rows_splat(L, r, stream));
    L->kn_rows64_splat = splat_rows_f64_launch(r->ptr.as<int>(), r->row.as<int>(), r->w.as<float>(), d_src, vd, (int)L->m,
                                               d_values, stream);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <bool VEC>
static void launch_slice_chunk_rows64(plx_lattice *L, const plx_lattice::RowsRange *r, const double2 *v2, int vd, int nch,
                                      double denom, double *d_out, hipStream_t stream)
{
    const int n = (int)L->n, d1 = L->d + 1, count = (int)r->count;
    const int shift = chunk_group_shift(nch);
    const int grid = ceil_div((int64_t)count << shift, kBlock);
    const int *pos = r->pos.as<int>(), *prow = r->prow.as<int>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    dispatch_d1(d1, [&](auto D1) {
        rows64_slice_chunk_kernel<VEC, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, count,
                                                                                         v2, vd, nch, shift, denom, d_out);
    });
}

int slice_rows_f64_impl(plx_lattice *L, const double *d_values, int vd, int64_t begin, int64_t count, double *d_out,
                        hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, begin, count);
    PLX_TRY(ensure_rows_slice(L, r, stream));
    const int n = (int)L->n, d1 = L->d + 1, nch = values_stride_f64(vd) / 2;
    const double denom = 1.0 + ldexp(1.0, -L->d);
    const int *pos = r->pos.as<int>(), *prow = r->prow.as<int>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const bool vec = f64_vec_ok(d_out, vd);
    const double2 *v2 = reinterpret_cast<const double2 *>(d_values);
    if (vd == 1) {
        L->kn_rows64_slice = "rows64_slice_v1_kernel";
        const int grid = ceil_div(count, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            rows64_slice_v1_kernel<decltype(D1)::value><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, (int)count,
                                                                                     d_values, denom, d_out);
        });
    } else if (nch <= kChunkGroupMax) {
        L->kn_rows64_slice = "rows64_slice_chunk_kernel";
        if (vec) launch_slice_chunk_rows64<true>(L, r, v2, vd, nch, denom, d_out, stream);
        else launch_slice_chunk_rows64<false>(L, r, v2, vd, nch, denom, d_out, stream);
    } else {
        L->kn_rows64_slice = "rows64_slice_wide_kernel";
        const int grid = ceil_div(count, kBlock / 64);
        if (vec)
            rows64_slice_wide_kernel<true><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, (int)count, v2, vd, nch,
                                                                        denom, d_out);
        else
            rows64_slice_wide_kernel<false><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, (int)count, v2, vd, nch,
                                                                         denom, d_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
