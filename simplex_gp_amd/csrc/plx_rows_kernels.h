// plx_rows_kernels.h -- the splat and the slice of the rectangular product K[out rows, src rows] v, restricted to a range of
// the caller's rows (plx_splat_rows / plx_slice_rows / plx_apply_rows and the same three with _f64, include/plx.h; the entry
// points and their argument checks are in plx_api.hip).  One templated source for fp32 and for double, instantiated by
// plx_rows.hip (float, next to the range tables both types share) and plx_rows_f64.hip (double): each holds the trait Rows<T>
// of its type, the names it reports.  What the types compute differently is Gather<T> (plx_kernels.h).  The blur in the
// middle is plx_blur's or plx_f64.hip's.
//
// Kernels (256-thread workgroups, wave64; value rows are whole 16-byte chunks, plx_kernels.h):
//   rows_splat_v1_kernel     vd = 1: one thread per vertex adds up the range's corners there, in order;
//   rows_splat_chunk_kernel  1..64 chunks per row: a group of G = 2^k >= chunks lanes per vertex, one lane per chunk;
//   rows_splat_wide_kernel   more than 64 chunks: one wave per vertex, its lanes stride over the chunks;
//   rows_slice_v1_kernel / rows_slice_chunk_kernel / rows_slice_wide_kernel: the same three shapes per entry j of the
//                            range's position table, p = pos[j] in ascending lattice order, stored to out[prow[j]].
// Every vertex row is written by exactly one thread per chunk (zero where the range has no corner there): no atomics, no
// zero-fill pass, bitwise reproducible.  Why the gates sit at 1 and 64 chunks: DESIGN.md section 13.
//
// In double the arithmetic is that of plx_f64.hip, formed from the same pieces in the same order: a range's corner table is
// a stable compaction of the vertex-sorted corners, so a vertex row keeps the order of its surviving terms, and a term
// dropped here is fma(w, 0, acc) = acc there.  Hence plx_apply_rows_f64 equals, as values, the wanted rows of plx_apply_f64
// of the zero-padded right-hand side.
//
// The kernels report as rows_*_kernel (plx_last_rows_kernels) and rows64_*_kernel (plx_last_rows_f64_kernels); the symbols a
// profiler shows are rows_*_kernel<float, ...> and rows_*_kernel<double, ...>.
#pragma once
#include "plx_kernels.h"

namespace plx {

// the lattice's two report fields (kSplatField / kSliceField) and the six names: kSplatV1 / kSplatChunk / kSplatWide,
// kSliceV1 / kSliceChunk / kSliceWide
template <typename T> struct Rows;

// ---- splat ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void rows_splat_v1_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                               const float *__restrict__ w, const T *__restrict__ src, int m,
                                                               T *__restrict__ values)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    T acc = T(0);
    for (int j = ptr[v], j1 = ptr[v + 1]; j < j1; ++j) acc += (T)w[j] * src[row[j]];
    values[v] = acc;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void rows_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                  const float *__restrict__ w, const T *__restrict__ src, int vd,
                                                                  int nch, int shift, int m,
                                                                  typename Gather<T>::Vec *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = Gather<T>::template vertex_sum<VEC>(row, w, ptr[v], ptr[v + 1], src, vd, ch);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void rows_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                 const float *__restrict__ w, const T *__restrict__ src, int vd,
                                                                 int nch, int m, typename Gather<T>::Vec *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = Gather<T>::template vertex_sum<VEC>(row, w, j0, j1, src, vd, ch);
}

// ---- slice (D1 > 0: d + 1 compiled in; 0: the run-time form) -------------------------------------------------------
template <typename T, int D1>
__global__ __launch_bounds__(kBlock) void rows_slice_v1_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                               const int *__restrict__ evid, const float *__restrict__ ew, int n,
                                                               int d1, int count, const T *__restrict__ values,
                                                               typename Gather<T>::Den den, T *__restrict__ out)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    out[prow[j]] = Gather<T>::template v1<D1, false>(evid, ew, n, pos[j], d1, values, den);
}

template <typename T, bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void rows_slice_chunk_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                                  const int *__restrict__ evid, const float *__restrict__ ew,
                                                                  int n, int d1, int count,
                                                                  const typename Gather<T>::Vec *__restrict__ values, int vd,
                                                                  int nch, int shift, typename Gather<T>::Den den,
                                                                  T *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (j >= count || ch >= nch) return;
    const typename Gather<T>::Vec acc = Gather<T>::template chunk<D1, false>(evid, ew, n, pos[j], d1, values, nch, ch, den);
    Gather<T>::template store<VEC>(out, (size_t)prow[j], vd, ch, acc);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void rows_slice_wide_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                                 const int *__restrict__ evid, const float *__restrict__ ew,
                                                                 int n, int d1, int count,
                                                                 const typename Gather<T>::Vec *__restrict__ values, int vd,
                                                                 int nch, typename Gather<T>::Den den, T *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (j >= count) return;
    const int p = pos[j];
    const size_t row = (size_t)prow[j];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        Gather<T>::template store<VEC>(out, row, vd, ch,
                                       Gather<T>::template wide<false>(evid, ew, n, p, d1, values, nch, ch, den));
}

// ---- launch side (kChunkGroupMax / chunk_group_shift: plx_kernels.h) -----------------------------------------------
template <typename T>
const char *splat_rows_launch(const int *ptr, const int *row, const float *w, const T *d_src, int vd, int m, T *d_values,
                              hipStream_t stream)
{
    using G = Gather<T>;
    const int nch = G::stride(vd) / G::kPer;
    const bool vec = G::vec_ok(d_src, vd);
    typename G::Vec *vv = reinterpret_cast<typename G::Vec *>(d_values);
    if (vd == 1) {
        rows_splat_v1_kernel<T><<<ceil_div(m, kBlock), kBlock, 0, stream>>>(ptr, row, w, d_src, m, d_values);
        return Rows<T>::kSplatV1;
    }
    if (nch <= kChunkGroupMax) {
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        if (vec) rows_splat_chunk_kernel<T, true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, vv);
        else rows_splat_chunk_kernel<T, false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, vv);
        return Rows<T>::kSplatChunk;
    }
    const int grid = ceil_div(m, kBlock / 64);
    if (vec) rows_splat_wide_kernel<T, true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, vv);
    else rows_splat_wide_kernel<T, false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, vv);
    return Rows<T>::kSplatWide;
}

template <typename T>
int splat_rows_impl(plx_lattice *L, const T *d_src, int64_t begin, int64_t count, int vd, T *d_values, hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, begin, count);
    PLX_TRY(ensure_rows_splat(L, r, stream));
    L->*Rows<T>::kSplatField = splat_rows_launch<T>(r->ptr.as<int>(), r->row.as<int>(), r->w.as<float>(), d_src, vd, (int)L->m,
                                                    d_values, stream);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <typename T>
int slice_rows_impl(plx_lattice *L, const T *d_values, int vd, int64_t begin, int64_t count, T *d_out, hipStream_t stream)
{
    using G = Gather<T>;
    plx_lattice::RowsRange *r = range_slot(L, begin, count);
    PLX_TRY(ensure_rows_slice(L, r, stream));
    const int n = (int)L->n, d1 = L->d + 1, cnt = (int)count, nch = G::stride(vd) / G::kPer;
    const typename G::Den den = G::den(L);
    const int *pos = r->pos.as<int>(), *prow = r->prow.as<int>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const bool vec = G::vec_ok(d_out, vd);
    const typename G::Vec *vv = reinterpret_cast<const typename G::Vec *>(d_values);
    if (vd == 1) {
        L->*Rows<T>::kSliceField = Rows<T>::kSliceV1;
        const int grid = ceil_div(count, kBlock);
        if constexpr (G::kV1Compiled) {
            dispatch_d1(d1, [&](auto D1) {
                rows_slice_v1_kernel<T, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, cnt, d_values,
                                                                                          den, d_out);
            });
        } else {
            rows_slice_v1_kernel<T, 0><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, cnt, d_values, den, d_out);
        }
    } else if (nch <= kChunkGroupMax) {
        L->*Rows<T>::kSliceField = Rows<T>::kSliceChunk;
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div(count << shift, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            if (vec)
                rows_slice_chunk_kernel<T, true, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, cnt,
                                                                                                   vv, vd, nch, shift, den, d_out);
            else
                rows_slice_chunk_kernel<T, false, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, cnt,
                                                                                                    vv, vd, nch, shift, den, d_out);
        });
    } else {
        L->*Rows<T>::kSliceField = Rows<T>::kSliceWide;
        const int grid = ceil_div(count, kBlock / 64);
        if (vec) rows_slice_wide_kernel<T, true><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, cnt, vv, vd, nch, den, d_out);
        else rows_slice_wide_kernel<T, false><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1, cnt, vv, vd, nch, den, d_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
