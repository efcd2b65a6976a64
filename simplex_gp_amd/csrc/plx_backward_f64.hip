// plx_backward_f64.hip -- the float64 position gradient of out = K(x) src on a lattice built with the DERIVATIVE taps:
// plx_backward_splat_f64 / plx_backward_contract_f64 / plx_apply_backward_f64 (include/plx.h; the entry points and their
// argument checks are in plx_api.hip).  bilateral_kernel.py:113-123 in double without its two big matrices: the stacked
// matrix [ g | g (x) x | src | src (x) x ] is formed inside the splat, the contraction of the filtered stack inside the
// slice.  The blur between them is blur_f64_impl (plx_f64.hip), unchanged, at width C.
//
// L = nrhs columns, C = 2 L (1 + d) stack columns (always even), nch = C / 2 = L (1 + d) double2 chunks per value row.
// Column c of the stack, tests/lattice64.py::stack64: h = L (1 + d); c < h comes from g, c >= h from src (c -= h); then
// c < L is the plain column l = c, else the product column (l, k) = divmod(c - L, d): l-major.  x is the caller's float64
// position matrix [n][d], not the float32 copy the lattice was built on.
//
// Kernels (256-thread workgroups, wave64), the chunk / wide shapes of plx_f64.hip:
//   f64_backward_splat_chunk_kernel / f64_backward_splat_wide_kernel   f64_splat_chunk_kernel / f64_splat_wide_kernel with
//       the source chunk formed on the fly: a lane decodes its two columns once, then per corner reads a = (g | src)[row][l]
//       and, for a product column, x[row][k], forms the element as ONE rounded multiply a * x and accumulates
//       fma((double)w, element, acc) in the corner order of f64_vertex_sum.
//   f64_backward_contract_chunk_kernel / f64_backward_contract_wide_kernel   a lane group (a wave) per point in LATTICE order
//       forms the point's filtered row with the sums of the fp64 slices -- d + 1 compiled in up to kGatherMaxD1, the run-time
//       form above, one division by 1 + 2^-d -- and keeps it in LDS: 16 bytes per lane (chunk), nch * 16 bytes per wave
//       (wide, dynamic).  A row never leaves its wave.  From the row, lane k < d of the group writes
//           grad_x[row][k] = -2 sum_l ( s_l x_k wg_l - s_l wgx_lk + g_l x_k ws_l - g_l wsx_lk )
//       with the sum taken for l ascending and the four terms in the order written, starting from 0, each product s_l x_k
//       and g_l x_k formed first; lane l < L writes grad_src[row][l] = wg_l.  Both go to the caller's row through the
//       point permutation.
// The wide shape holds 4 rows of C doubles in the 64 KiB of LDS a workgroup may have: C <= kBackwardF64MaxCols = 2048.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, bitwise reproducible.

#include "plx_kernels.h"

#include <math.h>

namespace plx {

// (the stack element and its vertex sum -- StackCol64, stack_col64, stack_elem64, stack_vertex_sum64 -- are in plx_kernels.h,
// shared with the trait of plx_rows_backward_f64.hip; the one-sided form's kernels are the templates of
// plx_rows_backward_kernels.h, this file's have the same skeleton over two inputs and the point permutation)
__global__ __launch_bounds__(kBlock) void f64_backward_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                          const float *__restrict__ w, const double *__restrict__ g,
                                                                          const double *__restrict__ src, const double *__restrict__ x,
                                                                          int L, int d, int nch, int shift, int m,
                                                                          double2 *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = stack_vertex_sum64(row, w, ptr[v], ptr[v + 1], g, src, x, L, d, ch);
}

__global__ __launch_bounds__(kBlock) void f64_backward_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                         const float *__restrict__ w, const double *__restrict__ g,
                                                                         const double *__restrict__ src, const double *__restrict__ x,
                                                                         int L, int d, int nch, int m, double2 *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = stack_vertex_sum64(row, w, j0, j1, g, src, x, L, d, ch);
}

// ---- slice + contraction -------------------------------------------------------------------------------------------
// (the corners of a point and the chunk of its filtered row -- Corners64, filtered_chunk64 -- are in plx_kernels.h)
// f: the point's filtered row [ wg | wgx | ws | wsx ] of C doubles in LDS.  Lane `lane` of `lanes` takes k = lane, lane +
// lanes, ... and then l likewise: every output element has one writer.
__device__ __forceinline__ void contract_row64(const double *f, int lane, int lanes, size_t row, const double *__restrict__ g,
                                               const double *__restrict__ src, const double *__restrict__ x, int L, int d,
                                               double *__restrict__ grad_x, double *__restrict__ grad_src)
{
    const int h = L * (1 + d);
    for (int k = lane; k < d; k += lanes) {
        const double xk = x[row * d + k];
        double acc = 0.0;
        for (int l = 0; l < L; ++l) {
            const double s = src[row * L + l], gl = g[row * L + l];
            acc += (s * xk) * f[l];
            acc -= s * f[L + l * d + k];
            acc += (gl * xk) * f[h + l];
            acc -= gl * f[h + L + l * d + k];
        }
        grad_x[row * d + k] = -2.0 * acc;
    }
    if (grad_src)
        for (int l = lane; l < L; l += lanes) grad_src[row * L + l] = f[l];
}

template <int D1>
__global__ __launch_bounds__(kBlock) void f64_backward_contract_chunk_kernel(
    const uint32_t *__restrict__ perm, const int *__restrict__ evid, const float *__restrict__ ew, int n, int d1,
    const double2 *__restrict__ values, int nch, int shift, double denom, const double *__restrict__ g,
    const double *__restrict__ src, const double *__restrict__ x, int L, int d, double *__restrict__ grad_x,
    double *__restrict__ grad_src)
{
    __shared__ double2 rows[kBlock];                  // one chunk per lane; a group's row starts at its first lane
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t p64 = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));     // kBlock is a multiple of the group: also the lane's place in the group
    const bool live = p64 < n;
    const int p = live ? (int)p64 : 0;
    if (live && ch < nch) {
        Corners64<D1> c;
        c.load(evid, ew, n, p);
        rows[threadIdx.x] = filtered_chunk64<D1>(c, evid, ew, n, p, d1, values, nch, ch, denom);
    }
    __syncthreads();                                  // every thread of the workgroup arrives: nothing has returned yet
    if (!live) return;
    contract_row64(reinterpret_cast<const double *>(rows + (threadIdx.x - ch)), ch, 1 << shift, (size_t)perm[p], g, src, x, L,
                   d, grad_x, grad_src);
}

template <int D1>
__global__ __launch_bounds__(kBlock) void f64_backward_contract_wide_kernel(
    const uint32_t *__restrict__ perm, const int *__restrict__ evid, const float *__restrict__ ew, int n, int d1,
    const double2 *__restrict__ values, int nch, double denom, const double *__restrict__ g, const double *__restrict__ src,
    const double *__restrict__ x, int L, int d, double *__restrict__ grad_x, double *__restrict__ grad_src)
{
    extern __shared__ double2 wide_rows[];            // kBlock / 64 rows of nch chunks, one per wave
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t p64 = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    const bool live = p64 < n;
    const int p = live ? (int)p64 : 0;
    double2 *mine = wide_rows + (size_t)wave * nch;
    if (live) {
        Corners64<D1> c;
        c.load(evid, ew, n, p);
        for (int ch = lane; ch < nch; ch += 64) mine[ch] = filtered_chunk64<D1>(c, evid, ew, n, p, d1, values, nch, ch, denom);
    }
    __syncthreads();
    if (!live) return;
    contract_row64(reinterpret_cast<const double *>(mine), lane, 64, (size_t)perm[p], g, src, x, L, d, grad_x, grad_src);
}

// ---- launch side ---------------------------------------------------------------------------------------------------
// the vertex-sorted corners and their row pointer, as the fp64 splat of plx_f64.hip keeps them (the same generation mark)
static int ensure_backward_tables(plx_lattice *L, hipStream_t stream)
{
    if (L->f64_gen == L->build_gen) return PLX_OK;
    PLX_TRY(refuse_under_capture(stream, "the vertex row pointer of the float64 splat"));
    PLX_TRY(export_row_ptr(L, stream));
    L->f64_gen = L->build_gen;
    return PLX_OK;
}

int backward_splat_f64_impl(plx_lattice *L, const double *d_g, const double *d_src, const double *d_x, int nrhs,
                            double *d_values, hipStream_t stream)
{
    PLX_TRY(ensure_backward_tables(L, stream));
    const int m = (int)L->m, d = L->d, nch = nrhs * (1 + d);
    const int *ptr = L->row_ptr.as<int>(), *row = L->csr_row.as<int>();
    const float *w = L->csr_w.as<float>();
    double2 *v2 = reinterpret_cast<double2 *>(d_values);
    if (nch <= kChunkGroupMax) {
        L->kn_f64_splat = "f64_backward_splat_chunk_kernel";
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        f64_backward_splat_chunk_kernel<<<grid, kBlock, 0, stream>>>(ptr, row, w, d_g, d_src, d_x, nrhs, d, nch, shift, m, v2);
    } else {
        L->kn_f64_splat = "f64_backward_splat_wide_kernel";
        const int grid = ceil_div(m, kBlock / 64);
        f64_backward_splat_wide_kernel<<<grid, kBlock, 0, stream>>>(ptr, row, w, d_g, d_src, d_x, nrhs, d, nch, m, v2);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

int backward_contract_f64_impl(plx_lattice *L, const double *d_values, const double *d_g, const double *d_src,
                               const double *d_x, int nrhs, double *d_grad_x, double *d_grad_src, hipStream_t stream)
{
    const int n = (int)L->n, d = L->d, d1 = d + 1, nch = nrhs * (1 + d);
    const double denom = 1.0 + ldexp(1.0, -d);
    const uint32_t *perm = L->perm.as<uint32_t>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const double2 *v2 = reinterpret_cast<const double2 *>(d_values);
    if (nch <= kChunkGroupMax) {
        L->kn_f64_slice = "f64_backward_contract_chunk_kernel";
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div((int64_t)n << shift, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            f64_backward_contract_chunk_kernel<decltype(D1)::value><<<grid, kBlock, 0, stream>>>(
                perm, evid, ew, n, d1, v2, nch, shift, denom, d_g, d_src, d_x, nrhs, d, d_grad_x, d_grad_src);
        });
    } else {
        L->kn_f64_slice = "f64_backward_contract_wide_kernel";
        const int grid = ceil_div(n, kBlock / 64);
        const size_t lds = (size_t)(kBlock / 64) * nch * sizeof(double2);      // <= 64 KiB: nch <= kBackwardF64MaxCols / 2
        dispatch_d1(d1, [&](auto D1) {
            f64_backward_contract_wide_kernel<decltype(D1)::value><<<grid, kBlock, lds, stream>>>(
                perm, evid, ew, n, d1, v2, nch, denom, d_g, d_src, d_x, nrhs, d, d_grad_x, d_grad_src);
        });
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
