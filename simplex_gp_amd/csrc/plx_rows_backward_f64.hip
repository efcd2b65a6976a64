// plx_rows_backward_f64.hip -- the float64 position gradient of the rectangular product out = K[out rows, src rows] src on a
// lattice built with the DERIVATIVE taps, one side at a time: plx_backward_splat_rows_f64 / plx_backward_contract_rows_f64 /
// plx_apply_backward_rows_f64 (include/plx.h; the entry points and their argument checks are in plx_api.hip).
//
// With G the incoming gradient (non-zero on the out rows only) and S the right-hand side (non-zero on the source rows only)
// the four terms of bilateral_kernel.py:113-123 fall apart: on the source rows only s_l x_k wg_l - s_l wgx_lk lives, on the
// out rows only g_l x_k ws_l - g_l wsx_lk.  Each is ONE one-sided call (a, b):
//     [ wa | wax ] = K[b rows, a rows] [ a | a (x) x ],     grad_x[i][k] = -2 sum_l ( (b_l x_k) wa_l - b_l wax_lk ),  i in b rows
// a row-range product of H = L (1 + d) columns -- half the padded stack -- whose stack is formed inside the splat and whose
// filtered image is contracted inside the slice, as plx_backward_f64.hip does for the square gradient.  The blur between
// them is blur_f64_impl (plx_f64.hip), unchanged, at width H.
//
// L = nrhs, H = L (1 + d) >= 2, stride = H rounded up to even, nch = stride / 2 double2 chunks per value row.  Column c of
// the half stack: c < L is the plain column l = c, else the product column (l, k) = divmod(c - L, d), l-major; the padding
// column of an odd H is 0.  x is the caller's float64 position matrix [n][d] of ALL stacked points; a is [a_count][L] on rows
// [a_begin, a_begin + a_count), b is [b_count][L] on rows [b_begin, b_begin + b_count).  The tables are the RowsRange slots of
// plx_rows.hip (ptr / row / w per vertex, pos / prow per point, rows counted from the range's first): nothing new is stored.
//
// Kernels (256-thread workgroups, wave64), the two shapes of plx_backward_f64.hip over the tables of plx_rows_f64.hip:
//   rows64_backward_splat_chunk_kernel / rows64_backward_splat_wide_kernel   a lane group (a wave) per vertex over the range's
//       compacted corner table: a lane decodes its two columns once, then per corner forms the element as ONE rounded
//       multiply a * x (plain columns are copied) and accumulates fma((double)w, element, acc) in the table's corner order.
//       Every vertex row is written, 0 where the range has no corner: no zero-fill pass.
//   rows64_backward_contract_chunk_kernel / rows64_backward_contract_wide_kernel   a lane group (a wave) per entry j of the
//       range's position table (p = pos[j], ascending lattice order) forms the filtered row with the sums of the fp64 slices
//       -- d + 1 compiled in up to kGatherMaxD1, the run-time form above, one division by 1 + 2^-d -- and keeps it in LDS:
//       16 bytes per lane (chunk), nch * 16 bytes per wave (wide, dynamic).  A row never leaves its wave.  Lane k < d writes
//       grad_x[prow[j]][k], the sum started at 0, taken for l ascending, the two terms in the order written, b_l x_k formed
//       first; lane l < L writes filtered[prow[j]][l] = wa_l.
// The wide shape holds 4 rows of `stride` doubles in the 64 KiB of LDS a workgroup may have: stride <= kBackwardF64MaxCols.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, bitwise reproducible.

#include "plx_kernels.h"

#include <math.h>

namespace plx {

// stack_vertex_sum64 over chunk ch of the HALF stack [ a | a (x) x ]: both halves of the square stack's column decoder point
// at a, so every column c < H decodes as the square stack's column c; the padding column of an odd H is set to 0
__device__ __forceinline__ double2 half_stack_vertex_sum64(const int *__restrict__ row, const float *__restrict__ w, int j0, int j1,
                                                           const double *__restrict__ a, const double *__restrict__ x, int L, int d,
                                                           int ch)
{
    double2 acc = stack_vertex_sum64(row, w, j0, j1, a, a, x, L, d, ch);
    if (2 * ch + 1 >= L * (1 + d)) acc.y = 0.0;
    return acc;
}

__global__ __launch_bounds__(kBlock) void rows64_backward_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                             const float *__restrict__ w, const double *__restrict__ a,
                                                                             const double *__restrict__ x, int L, int d, int nch,
                                                                             int shift, int m, double2 *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = half_stack_vertex_sum64(row, w, ptr[v], ptr[v + 1], a, x, L, d, ch);
}

__global__ __launch_bounds__(kBlock) void rows64_backward_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                            const float *__restrict__ w, const double *__restrict__ a,
                                                                            const double *__restrict__ x, int L, int d, int nch, int m,
                                                                            double2 *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = half_stack_vertex_sum64(row, w, j0, j1, a, x, L, d, ch);
}

// ---- slice + contraction -------------------------------------------------------------------------------------------
// f: the filtered row [ wa | wax ] of H doubles in LDS.  Lane `lane` of `lanes` takes k = lane, lane + lanes, ... and then l
// likewise: every output element has one writer.  b, x, grad_x and filtered start at the range's first row.
__device__ __forceinline__ void contract_half_row64(const double *f, int lane, int lanes, size_t row, const double *__restrict__ b,
                                                    const double *__restrict__ x, int L, int d, double *__restrict__ grad_x,
                                                    double *__restrict__ filtered)
{
    for (int k = lane; k < d; k += lanes) {
        const double xk = x[row * d + k];
        double acc = 0.0;
        for (int l = 0; l < L; ++l) {
            const double bl = b[row * L + l];
            acc += (bl * xk) * f[l];
            acc -= bl * f[L + l * d + k];
        }
        grad_x[row * d + k] = -2.0 * acc;
    }
    if (filtered)
        for (int l = lane; l < L; l += lanes) filtered[row * L + l] = f[l];
}

template <int D1>
__global__ __launch_bounds__(kBlock) void rows64_backward_contract_chunk_kernel(
    const int *__restrict__ pos, const int *__restrict__ prow, const int *__restrict__ evid, const float *__restrict__ ew, int n,
    int d1, int count, const double2 *__restrict__ values, int nch, int shift, double denom, const double *__restrict__ b,
    const double *__restrict__ x, int L, int d, double *__restrict__ grad_x, double *__restrict__ filtered)
{
    __shared__ double2 rows[kBlock];                  // one chunk per lane; a group's row starts at its first lane
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j64 = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));     // kBlock is a multiple of the group: also the lane's place in the group
    const bool live = j64 < count;
    const int j = live ? (int)j64 : 0;
    if (live && ch < nch) {
        const int p = pos[j];
        Corners64<D1> c;
        c.load(evid, ew, n, p);
        rows[threadIdx.x] = filtered_chunk64<D1>(c, evid, ew, n, p, d1, values, nch, ch, denom);
    }
    __syncthreads();                                  // every thread of the workgroup arrives: nothing has returned yet
    if (!live) return;
    contract_half_row64(reinterpret_cast<const double *>(rows + (threadIdx.x - ch)), ch, 1 << shift, (size_t)prow[j], b, x, L, d,
                        grad_x, filtered);
}

template <int D1>
__global__ __launch_bounds__(kBlock) void rows64_backward_contract_wide_kernel(
    const int *__restrict__ pos, const int *__restrict__ prow, const int *__restrict__ evid, const float *__restrict__ ew, int n,
    int d1, int count, const double2 *__restrict__ values, int nch, double denom, const double *__restrict__ b,
    const double *__restrict__ x, int L, int d, double *__restrict__ grad_x, double *__restrict__ filtered)
{
    extern __shared__ double2 wide_rows[];            // kBlock / 64 rows of nch chunks, one per wave
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j64 = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    const bool live = j64 < count;
    const int j = live ? (int)j64 : 0;
    double2 *mine = wide_rows + (size_t)wave * nch;
    if (live) {
        const int p = pos[j];
        Corners64<D1> c;
        c.load(evid, ew, n, p);
        for (int ch = lane; ch < nch; ch += 64) mine[ch] = filtered_chunk64<D1>(c, evid, ew, n, p, d1, values, nch, ch, denom);
    }
    __syncthreads();
    if (!live) return;
    contract_half_row64(reinterpret_cast<const double *>(mine), lane, 64, (size_t)prow[j], b, x, L, d, grad_x, filtered);
}

// ---- launch side ---------------------------------------------------------------------------------------------------
// Both tables of a call, before its first launch: under stream capture a table that is missing refuses here, with nothing
// captured yet.  The slot of the a range is the most recently used when the b range is looked up, so it is never recycled.
int backward_rows_f64_tables(plx_lattice *L, int64_t a_begin, int64_t a_count, int64_t b_begin, int64_t b_count,
                             hipStream_t stream)
{
    PLX_TRY(ensure_rows_splat(L, range_slot(L, a_begin, a_count), stream));
    return ensure_rows_slice(L, range_slot(L, b_begin, b_count), stream);
}

int backward_splat_rows_f64_impl(plx_lattice *L, const double *d_a, int64_t a_begin, int64_t a_count, const double *d_x, int nrhs,
                                 double *d_values, hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, a_begin, a_count);
    PLX_TRY(ensure_rows_splat(L, r, stream));
    const int m = (int)L->m, d = L->d, nch = values_stride_f64(nrhs * (1 + d)) / 2;
    const int *ptr = r->ptr.as<int>(), *row = r->row.as<int>();
    const float *w = r->w.as<float>();
    const double *x = d_x + (size_t)a_begin * d;      // the table's rows count from a_begin
    double2 *v2 = reinterpret_cast<double2 *>(d_values);
    if (nch <= kF64ChunkMax) {
        L->kn_rows64_splat = "rows64_backward_splat_chunk_kernel";
        const int shift = f64_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        rows64_backward_splat_chunk_kernel<<<grid, kBlock, 0, stream>>>(ptr, row, w, d_a, x, nrhs, d, nch, shift, m, v2);
    } else {
        L->kn_rows64_splat = "rows64_backward_splat_wide_kernel";
        const int grid = ceil_div(m, kBlock / 64);
        rows64_backward_splat_wide_kernel<<<grid, kBlock, 0, stream>>>(ptr, row, w, d_a, x, nrhs, d, nch, m, v2);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

int backward_contract_rows_f64_impl(plx_lattice *L, const double *d_values, const double *d_b, int64_t b_begin, int64_t b_count,
                                    const double *d_x, int nrhs, double *d_grad_x, double *d_filtered, hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, b_begin, b_count);
    PLX_TRY(ensure_rows_slice(L, r, stream));
    const int n = (int)L->n, d = L->d, d1 = d + 1, count = (int)b_count, nch = values_stride_f64(nrhs * (1 + d)) / 2;
    const double denom = 1.0 + ldexp(1.0, -d);
    const int *pos = r->pos.as<int>(), *prow = r->prow.as<int>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const double *x = d_x + (size_t)b_begin * d;      // the table's rows count from b_begin
    const double2 *v2 = reinterpret_cast<const double2 *>(d_values);
    if (nch <= kF64ChunkMax) {
        L->kn_rows64_slice = "rows64_backward_contract_chunk_kernel";
        const int shift = f64_group_shift(nch);
        const int grid = ceil_div((int64_t)count << shift, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            rows64_backward_contract_chunk_kernel<decltype(D1)::value><<<grid, kBlock, 0, stream>>>(
                pos, prow, evid, ew, n, d1, count, v2, nch, shift, denom, d_b, x, nrhs, d, d_grad_x, d_filtered);
        });
    } else {
        L->kn_rows64_slice = "rows64_backward_contract_wide_kernel";
        const int grid = ceil_div(count, kBlock / 64);
        const size_t lds = (size_t)(kBlock / 64) * nch * sizeof(double2);      // <= 64 KiB: nch <= kBackwardF64MaxCols / 2
        dispatch_d1(d1, [&](auto D1) {
            rows64_backward_contract_wide_kernel<decltype(D1)::value><<<grid, kBlock, lds, stream>>>(
                pos, prow, evid, ew, n, d1, count, v2, nch, denom, d_b, x, nrhs, d, d_grad_x, d_filtered);
        });
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
