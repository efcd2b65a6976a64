// plx_rows_backward_kernels.h -- the position gradient of the rectangular product out = K[out rows, src rows] src on a
// lattice built with the DERIVATIVE taps, one side at a time: plx_backward_splat_rows / plx_backward_contract_rows /
// plx_apply_backward_rows and the same three with _f64 (include/plx.h; the entry points and their argument checks are in
// plx_api.hip).  One templated source for fp32 and for double, instantiated by plx_rows_backward.hip (float) and
// plx_rows_backward_f64.hip (double): each holds the trait RowsBackward<T> of its type -- the device functions that round
// differently and the kernel names it reports -- and the explicit instantiations of the three launch-side functions.
//
// With G the incoming gradient (non-zero on the out rows only) and S the right-hand side (non-zero on the source rows only)
// the four terms of bilateral_kernel.py:113-123 fall apart: on the source rows only s_l x_k wg_l - s_l wgx_lk lives, on the
// out rows only g_l x_k ws_l - g_l wsx_lk.  Each is ONE one-sided call (a, b):
//     [ wa | wax ] = K[b rows, a rows] [ a | a (x) x ],     grad_x[i][k] = -2 sum_l ( (b_l x_k) wa_l - b_l wax_lk ),  i in b rows
// a row-range product of H = L (1 + d) columns -- half the padded stack -- whose stack is formed inside the splat and whose
// filtered image is contracted inside the slice, as plx_backward_f64.hip does for the square gradient.  The blur between
// them is unchanged, at width H: blur_impl (plx_blur.hip) or blur_f64_impl (plx_f64.hip).
//
// L = nrhs, H = L (1 + d) >= 2, P = 16 / sizeof(T) elements in a 16-byte chunk, stride = H rounded up to P, nch = stride / P
// chunks per value row.  Column c of the half stack: c < L is the plain column l = c, else the product column (l, k) =
// divmod(c - L, d), l-major; the padding columns H <= c < stride are 0.  x is the caller's position matrix [n][d] of ALL
// stacked points; a is [a_count][L] on rows [a_begin, a_begin + a_count), b is [b_count][L] on rows [b_begin, b_begin +
// b_count).  The tables are the RowsRange slots of plx_rows.hip (ptr / row / w per vertex, pos / prow per point, rows counted
// from the range's first): nothing new is stored, and the slots are shared by the rows calls of both types.
//
// Kernels (256-thread workgroups, wave64), the two shapes of plx_backward_f64.hip:
//   rows_backward_splat_chunk_kernel / rows_backward_splat_wide_kernel   a group of 2^s >= nch lanes (a wave, its lanes
//       striding over the chunks) per vertex over the range's compacted corner table: a lane decodes its P columns once,
//       then per corner forms each product element as ONE rounded multiply a * x (plain columns are copied, padding is 0)
//       and accumulates w[j] * element in the table's corner order.  Every vertex row is written, 0 where the range has no
//       corner: no zero-fill pass.
//   rows_backward_contract_chunk_kernel / rows_backward_contract_wide_kernel   a lane group (a wave) per entry j of the
//       range's position table (p = pos[j], ascending lattice order) forms the filtered row -- d + 1 compiled in up to
//       kGatherMaxD1, the run-time form above -- and keeps it in LDS: 16 bytes per lane (chunk), nch * 16 bytes per wave
//       (wide, dynamic).  A row never leaves its wave.  Lane k < d writes grad_x[prow[j]][k], the sum started at 0, taken
//       for l ascending, the two terms in the order written, b_l x_k formed first; lane l < L writes filtered[prow[j]][l] =
//       wa_l.
// The wide shape holds 4 rows of `stride` elements in the 64 KiB of LDS a workgroup may have: stride <= kMaxCols.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, bitwise reproducible.
//
// What the types differ in, all of it in RowsBackward<T> (the host-side constants in RowsBackwardHost<T>, plx_internal.h):
//   float:  float4 chunks, stride = values_stride(H) <= kBackwardRowsMaxCols = 4096.  The vertex sum is the expression of
//           Gather<float>::vertex_sum (plx_kernels.h), acc += w[j] * element with the product element an explicit __fmul_rn.  The
//           filtered chunk is rows_filtered_chunk (plx_kernels.h), which reads the point's corners itself, per chunk, and
//           multiplies every term by the rounded reciprocal 1.0f / slice_denom: the corners type is empty.
//   double: double2 chunks, stride = values_stride_f64(H) <= kBackwardF64MaxCols = 2048.  The vertex sum is
//           stack_vertex_sum64 (plx_kernels.h, shared with the square gradient so that both give the same bits),
//           fma((double)w, element, acc), with the padding column of an odd H masked to 0.  The corners of a point are read
//           once per lane (Corners64) and the filtered chunk is filtered_chunk64: the sum, then ONE division by 1 + 2^-d.
// One body for either pair would change roundings in one of the types.
//
// The kernels report as rows_backward_* (plx_last_rows_kernels) and rows64_backward_* (plx_last_rows_f64_kernels); the
// symbols a profiler shows are rows_backward_*<float> and rows_backward_*<double>.
#pragma once
#include "plx_kernels.h"

namespace plx {

// Chunk, Corners<D1>, half_stack_vertex_sum, slice_scale, filtered_chunk, the lattice's two report fields and the four names
template <typename T> struct RowsBackward;

template <typename T>
__global__ __launch_bounds__(kBlock) void rows_backward_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                           const float *__restrict__ w, const T *__restrict__ a,
                                                                           const T *__restrict__ x, int L, int d, int nch, int shift,
                                                                           int m, typename RowsBackward<T>::Chunk *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = RowsBackward<T>::half_stack_vertex_sum(row, w, ptr[v], ptr[v + 1], a, x, L, d, ch);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rows_backward_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                          const float *__restrict__ w, const T *__restrict__ a,
                                                                          const T *__restrict__ x, int L, int d, int nch, int m,
                                                                          typename RowsBackward<T>::Chunk *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = RowsBackward<T>::half_stack_vertex_sum(row, w, j0, j1, a, x, L, d, ch);
}

// ---- slice + contraction -------------------------------------------------------------------------------------------
// f: the filtered row [ wa | wax ] of H elements in LDS.  Lane `lane` of `lanes` takes k = lane, lane + lanes, ... and then l
// likewise: every output element has one writer.  b, x, grad_x and filtered start at the range's first row.
template <typename T>
__device__ __forceinline__ void contract_half_row(const T *f, int lane, int lanes, size_t row, const T *__restrict__ b,
                                                  const T *__restrict__ x, int L, int d, T *__restrict__ grad_x,
                                                  T *__restrict__ filtered)
{
    for (int k = lane; k < d; k += lanes) {
        const T xk = x[row * d + k];
        T acc = T(0);
        for (int l = 0; l < L; ++l) {
            const T bl = b[row * L + l];
            acc += (bl * xk) * f[l];
            acc -= bl * f[L + l * d + k];
        }
        grad_x[row * d + k] = T(-2) * acc;
    }
    if (filtered)
        for (int l = lane; l < L; l += lanes) filtered[row * L + l] = f[l];
}

template <typename T, int D1>
__global__ __launch_bounds__(kBlock) void rows_backward_contract_chunk_kernel(
    const int *__restrict__ pos, const int *__restrict__ prow, const int *__restrict__ evid, const float *__restrict__ ew, int n,
    int d1, int count, const typename RowsBackward<T>::Chunk *__restrict__ values, int nch, int shift, T scale,
    const T *__restrict__ b, const T *__restrict__ x, int L, int d, T *__restrict__ grad_x, T *__restrict__ filtered)
{
    using S = RowsBackward<T>;
    __shared__ typename S::Chunk rows[kBlock];        // one chunk per lane; a group's row starts at its first lane
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j64 = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));     // kBlock is a multiple of the group: also the lane's place in the group
    const bool live = j64 < count;
    const int j = live ? (int)j64 : 0;
    if (live && ch < nch) {
        const int p = pos[j];
        typename S::template Corners<D1> c;
        c.load(evid, ew, n, p);
        rows[threadIdx.x] = S::template filtered_chunk<D1>(c, evid, ew, n, p, d1, values, nch, ch, scale);
    }
    __syncthreads();                                  // every thread of the workgroup arrives: nothing has returned yet
    if (!live) return;
    contract_half_row<T>(reinterpret_cast<const T *>(rows + (threadIdx.x - ch)), ch, 1 << shift, (size_t)prow[j], b, x, L, d,
                         grad_x, filtered);
}

template <typename T, int D1>
__global__ __launch_bounds__(kBlock) void rows_backward_contract_wide_kernel(
    const int *__restrict__ pos, const int *__restrict__ prow, const int *__restrict__ evid, const float *__restrict__ ew, int n,
    int d1, int count, const typename RowsBackward<T>::Chunk *__restrict__ values, int nch, T scale, const T *__restrict__ b,
    const T *__restrict__ x, int L, int d, T *__restrict__ grad_x, T *__restrict__ filtered)
{
    using S = RowsBackward<T>;
    extern __shared__ typename S::Chunk wide_rows[];  // kBlock / 64 rows of nch chunks, one per wave
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j64 = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    const bool live = j64 < count;
    const int j = live ? (int)j64 : 0;
    typename S::Chunk *mine = wide_rows + (size_t)wave * nch;
    if (live) {
        const int p = pos[j];
        typename S::template Corners<D1> c;
        c.load(evid, ew, n, p);
        for (int ch = lane; ch < nch; ch += 64) mine[ch] = S::template filtered_chunk<D1>(c, evid, ew, n, p, d1, values, nch, ch, scale);
    }
    __syncthreads();
    if (!live) return;
    contract_half_row<T>(reinterpret_cast<const T *>(mine), lane, 64, (size_t)prow[j], b, x, L, d, grad_x, filtered);
}

// ---- launch side (kChunkGroupMax / chunk_group_shift: plx_kernels.h) -------------------------------------------------
// Both tables of a call, before its first launch: under stream capture a table that is missing refuses here, with nothing
// captured yet.  The slot of the a range is the most recently used when the b range is looked up, so it is never recycled.
template <typename T>
int backward_rows_tables(plx_lattice *L, int64_t a_begin, int64_t a_count, int64_t b_begin, int64_t b_count, hipStream_t stream)
{
    PLX_TRY(ensure_rows_splat(L, range_slot(L, a_begin, a_count), stream));
    return ensure_rows_slice(L, range_slot(L, b_begin, b_count), stream);
}

template <typename T>
int backward_splat_rows_impl(plx_lattice *L, const T *d_a, int64_t a_begin, int64_t a_count, const T *d_x, int nrhs, T *d_values,
                             hipStream_t stream)
{
    using S = RowsBackward<T>;
    plx_lattice::RowsRange *r = range_slot(L, a_begin, a_count);
    PLX_TRY(ensure_rows_splat(L, r, stream));
    const int m = (int)L->m, d = L->d, nch = S::stride(nrhs * (1 + d)) / S::kPack;
    const int *ptr = r->ptr.as<int>(), *row = r->row.as<int>();
    const float *w = r->w.as<float>();
    const T *x = d_x + (size_t)a_begin * d;           // the table's rows count from a_begin
    typename S::Chunk *values = reinterpret_cast<typename S::Chunk *>(d_values);
    if (nch <= kChunkGroupMax) {
        L->*S::kSplatField = S::kSplatChunk;
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        rows_backward_splat_chunk_kernel<T><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_a, x, nrhs, d, nch, shift, m, values);
    } else {
        L->*S::kSplatField = S::kSplatWide;
        const int grid = ceil_div(m, kBlock / 64);
        rows_backward_splat_wide_kernel<T><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_a, x, nrhs, d, nch, m, values);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <typename T>
int backward_contract_rows_impl(plx_lattice *L, const T *d_values, const T *d_b, int64_t b_begin, int64_t b_count, const T *d_x,
                                int nrhs, T *d_grad_x, T *d_filtered, hipStream_t stream)
{
    using S = RowsBackward<T>;
    plx_lattice::RowsRange *r = range_slot(L, b_begin, b_count);
    PLX_TRY(ensure_rows_slice(L, r, stream));
    const int n = (int)L->n, d = L->d, d1 = d + 1, count = (int)b_count, nch = S::stride(nrhs * (1 + d)) / S::kPack;
    const T scale = S::slice_scale(L);
    const int *pos = r->pos.as<int>(), *prow = r->prow.as<int>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const T *x = d_x + (size_t)b_begin * d;           // the table's rows count from b_begin
    const typename S::Chunk *values = reinterpret_cast<const typename S::Chunk *>(d_values);
    if (nch <= kChunkGroupMax) {
        L->*S::kSliceField = S::kContractChunk;
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div((int64_t)count << shift, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            rows_backward_contract_chunk_kernel<T, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(
                pos, prow, evid, ew, n, d1, count, values, nch, shift, scale, d_b, x, nrhs, d, d_grad_x, d_filtered);
        });
    } else {
        L->*S::kSliceField = S::kContractWide;
        const int grid = ceil_div(count, kBlock / 64);
        const size_t lds = (size_t)(kBlock / 64) * nch * sizeof(typename S::Chunk);       // <= 64 KiB: nch <= kMaxCols / kPack
        dispatch_d1(d1, [&](auto D1) {
            rows_backward_contract_wide_kernel<T, decltype(D1)::value><<<grid, kBlock, lds, stream>>>(
                pos, prow, evid, ew, n, d1, count, values, nch, scale, d_b, x, nrhs, d, d_grad_x, d_filtered);
        });
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
