// plx_rows_backward.hip -- the fp32 position gradient of the rectangular product out = K[out rows, src rows] src on a lattice
// built with the DERIVATIVE taps, one side at a time: plx_backward_splat_rows / plx_backward_contract_rows /
// plx_apply_backward_rows (include/plx.h; the entry points and their argument checks are in plx_api.hip).  The fp32
// counterpart of plx_rows_backward_f64.hip, with the conventions of plx_rows.hip.
//
// One one-sided call (a, b):
//     [ wa | wax ] = K[b rows, a rows] [ a | a (x) x ],     grad_x[i][k] = -2 sum_l ( (b_l x_k) wa_l - b_l wax_lk ),  i in b rows
// a row-range product of H = L (1 + d) columns -- half the padded stack -- whose stack is formed inside the splat and whose
// filtered image is contracted inside the slice.  The blur between them is blur_impl (plx_blur.hip), unchanged, at vd = H.
//
// L = nrhs, H = L (1 + d) >= 2, stride = plx_values_stride(H) = H rounded up to 4, nch = stride / 4 float4 chunks per value
// row.  Column c of the half stack: c < L is the plain column l = c, else the product column (l, k) = divmod(c - L, d),
// l-major; the padding columns H <= c < stride are 0.  x is the caller's position matrix [n][d] of ALL stacked points; a is
// [a_count][L] on rows [a_begin, a_begin + a_count), b is [b_count][L] on rows [b_begin, b_begin + b_count).  The tables are
// the RowsRange slots of plx_rows.hip (ptr / row / w per vertex, pos / prow per point, rows counted from the range's first):
// nothing new is stored, and the slots are shared with the rows calls and the float64 calls.
//
// Kernels (256-thread workgroups, wave64):
//   rows_backward_splat_chunk_kernel / rows_backward_splat_wide_kernel   a group of 2^s >= nch lanes (a wave, its lanes
//       striding over the chunks) per vertex over the range's compacted corner table: a lane decodes its four columns once,
//       then per corner forms each product element as ONE rounded multiply a * x (plain columns are copied, padding is 0)
//       and accumulates acc += w[j] * element in the table's corner order, the expression of rows_vertex_sum.  Every vertex
//       row is written, 0 where the range has no corner: no zero-fill pass.
//   rows_backward_contract_chunk_kernel / rows_backward_contract_wide_kernel   a lane group (a wave) per entry j of the
//       range's position table forms the filtered row with the sum of the fp32 row slices (rows_filtered_chunk, plx_kernels.h:
//       d + 1 compiled in up to kGatherMaxD1, the run-time form above) and keeps it in LDS: 16 bytes per lane (chunk),
//       nch * 16 bytes per wave (wide, dynamic).  A row never leaves its wave.  Lane k < d writes grad_x[prow[j]][k], the sum
//       started at 0, taken for l ascending, the two terms in the order written, b_l x_k formed first; lane l < L writes
//       filtered[prow[j]][l] = wa_l.
// The wide shape holds 4 rows of `stride` floats in the 64 KiB of LDS a workgroup may have: stride <= kBackwardRowsMaxCols.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, bitwise reproducible.

#include "plx_kernels.h"

namespace plx {

// One column of the half stack, decoded once per lane: l, and k >= 0 for a product column a_l * x_k, -1 for the plain column
// a_l, -2 for a padding column.
struct HalfCol {
    int l, k;
};

__device__ __forceinline__ HalfCol half_col(int c, int L, int d)
{
    HalfCol s;
    if (c >= L * (1 + d)) {
        s.l = 0;
        s.k = -2;
    } else if (c < L) {
        s.l = c;
        s.k = -1;
    } else {
        c -= L;
        s.l = c / d;
        s.k = c - s.l * d;
    }
    return s;
}

__device__ __forceinline__ float half_elem(const HalfCol &s, const float *__restrict__ a, const float *__restrict__ x, size_t row,
                                           int L, int d)
{
    if (s.k == -2) return 0.f;
    const float al = a[row * L + s.l];
    return s.k < 0 ? al : __fmul_rn(al, x[row * d + s.k]);
}

// rows_vertex_sum over chunk ch of the half stack rows: the same weights, the same corner order, the same expression
__device__ __forceinline__ float4 half_stack_vertex_sum(const int *__restrict__ row, const float *__restrict__ w, int j0, int j1,
                                                        const float *__restrict__ a, const float *__restrict__ x, int L, int d,
                                                        int ch)
{
    const HalfCol c0 = half_col(4 * ch, L, d), c1 = half_col(4 * ch + 1, L, d), c2 = half_col(4 * ch + 2, L, d),
                  c3 = half_col(4 * ch + 3, L, d);
    float4 acc = f4_zero();
    for (int j = j0; j < j1; ++j) {
        const float wj = w[j];
        const size_t r = (size_t)row[j];
        const float4 e = make_float4(half_elem(c0, a, x, r, L, d), half_elem(c1, a, x, r, L, d), half_elem(c2, a, x, r, L, d),
                                     half_elem(c3, a, x, r, L, d));
        acc.x += wj * e.x; acc.y += wj * e.y; acc.z += wj * e.z; acc.w += wj * e.w;
    }
    return acc;
}

__global__ __launch_bounds__(kBlock) void rows_backward_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                           const float *__restrict__ w, const float *__restrict__ a,
                                                                           const float *__restrict__ x, int L, int d, int nch,
                                                                           int shift, int m, float4 *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = half_stack_vertex_sum(row, w, ptr[v], ptr[v + 1], a, x, L, d, ch);
}

__global__ __launch_bounds__(kBlock) void rows_backward_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                          const float *__restrict__ w, const float *__restrict__ a,
                                                                          const float *__restrict__ x, int L, int d, int nch, int m,
                                                                          float4 *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = half_stack_vertex_sum(row, w, j0, j1, a, x, L, d, ch);
}

// ---- slice + contraction -------------------------------------------------------------------------------------------
// f: the filtered row [ wa | wax ] of H floats in LDS.  Lane `lane` of `lanes` takes k = lane, lane + lanes, ... and then l
// likewise: every output element has one writer.  b, x, grad_x and filtered start at the range's first row.
__device__ __forceinline__ void contract_half_row(const float *f, int lane, int lanes, size_t row, const float *__restrict__ b,
                                                  const float *__restrict__ x, int L, int d, float *__restrict__ grad_x,
                                                  float *__restrict__ filtered)
{
    for (int k = lane; k < d; k += lanes) {
        const float xk = x[row * d + k];
        float acc = 0.f;
        for (int l = 0; l < L; ++l) {
            const float bl = b[row * L + l];
            acc += (bl * xk) * f[l];
            acc -= bl * f[L + l * d + k];
        }
        grad_x[row * d + k] = -2.f * acc;
    }
    if (filtered)
        for (int l = lane; l < L; l += lanes) filtered[row * L + l] = f[l];
}

template <int D1>
__global__ __launch_bounds__(kBlock) void rows_backward_contract_chunk_kernel(
    const int *__restrict__ pos, const int *__restrict__ prow, const int *__restrict__ evid, const float *__restrict__ ew, int n,
    int d1, int count, const float4 *__restrict__ values, int nch, int shift, float rden, const float *__restrict__ b,
    const float *__restrict__ x, int L, int d, float *__restrict__ grad_x, float *__restrict__ filtered)
{
    __shared__ float4 rows[kBlock];                   // one chunk per lane; a group's row starts at its first lane
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j64 = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));     // kBlock is a multiple of the group: also the lane's place in the group
    const bool live = j64 < count;
    const int j = live ? (int)j64 : 0;
    if (live && ch < nch) rows[threadIdx.x] = rows_filtered_chunk<D1>(evid, ew, n, pos[j], d1, values, nch, ch, rden);
    __syncthreads();                                  // every thread of the workgroup arrives: nothing has returned yet
    if (!live) return;
    contract_half_row(reinterpret_cast<const float *>(rows + (threadIdx.x - ch)), ch, 1 << shift, (size_t)prow[j], b, x, L, d,
                      grad_x, filtered);
}

template <int D1>
__global__ __launch_bounds__(kBlock) void rows_backward_contract_wide_kernel(
    const int *__restrict__ pos, const int *__restrict__ prow, const int *__restrict__ evid, const float *__restrict__ ew, int n,
    int d1, int count, const float4 *__restrict__ values, int nch, float rden, const float *__restrict__ b,
    const float *__restrict__ x, int L, int d, float *__restrict__ grad_x, float *__restrict__ filtered)
{
    extern __shared__ float4 wide_rows[];             // kBlock / 64 rows of nch chunks, one per wave
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j64 = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    const bool live = j64 < count;
    const int j = live ? (int)j64 : 0;
    float4 *mine = wide_rows + (size_t)wave * nch;
    if (live) {
        const int p = pos[j];
        for (int ch = lane; ch < nch; ch += 64) mine[ch] = rows_filtered_chunk<D1>(evid, ew, n, p, d1, values, nch, ch, rden);
    }
    __syncthreads();
    if (!live) return;
    contract_half_row(reinterpret_cast<const float *>(mine), lane, 64, (size_t)prow[j], b, x, L, d, grad_x, filtered);
}

// ---- launch side ---------------------------------------------------------------------------------------------------
constexpr int kBackwardRowsChunkMax = 64;      // chunks one lane group can cover: a group never spans two waves

static inline int backward_rows_group_shift(int nch)
{
    int s = 0;
    while ((1 << s) < nch) ++s;
    return s;
}

// Both tables of a call, before its first launch: under stream capture a table that is missing refuses here, with nothing
// captured yet.  The slot of the a range is the most recently used when the b range is looked up, so it is never recycled.
int backward_rows_tables(plx_lattice *L, int64_t a_begin, int64_t a_count, int64_t b_begin, int64_t b_count, hipStream_t stream)
{
    PLX_TRY(ensure_rows_splat(L, range_slot(L, a_begin, a_count), stream));
    return ensure_rows_slice(L, range_slot(L, b_begin, b_count), stream);
}

int backward_splat_rows_impl(plx_lattice *L, const float *d_a, int64_t a_begin, int64_t a_count, const float *d_x, int nrhs,
                             float *d_values, hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, a_begin, a_count);
    PLX_TRY(ensure_rows_splat(L, r, stream));
    const int m = (int)L->m, d = L->d, nch = values_stride(nrhs * (1 + d)) / 4;
    const int *ptr = r->ptr.as<int>(), *row = r->row.as<int>();
    const float *w = r->w.as<float>();
    const float *x = d_x + (size_t)a_begin * d;       // the table's rows count from a_begin
    float4 *v4 = reinterpret_cast<float4 *>(d_values);
    if (nch <= kBackwardRowsChunkMax) {
        L->kn_rows_splat = "rows_backward_splat_chunk_kernel";
        const int shift = backward_rows_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        rows_backward_splat_chunk_kernel<<<grid, kBlock, 0, stream>>>(ptr, row, w, d_a, x, nrhs, d, nch, shift, m, v4);
    } else {
        L->kn_rows_splat = "rows_backward_splat_wide_kernel";
        const int grid = ceil_div(m, kBlock / 64);
        rows_backward_splat_wide_kernel<<<grid, kBlock, 0, stream>>>(ptr, row, w, d_a, x, nrhs, d, nch, m, v4);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

int backward_contract_rows_impl(plx_lattice *L, const float *d_values, const float *d_b, int64_t b_begin, int64_t b_count,
                                const float *d_x, int nrhs, float *d_grad_x, float *d_filtered, hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, b_begin, b_count);
    PLX_TRY(ensure_rows_slice(L, r, stream));
    const int n = (int)L->n, d = L->d, d1 = d + 1, count = (int)b_count, nch = values_stride(nrhs * (1 + d)) / 4;
    const float rden = 1.0f / L->slice_denom;
    const int *pos = r->pos.as<int>(), *prow = r->prow.as<int>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const float *x = d_x + (size_t)b_begin * d;       // the table's rows count from b_begin
    const float4 *v4 = reinterpret_cast<const float4 *>(d_values);
    if (nch <= kBackwardRowsChunkMax) {
        L->kn_rows_slice = "rows_backward_contract_chunk_kernel";
        const int shift = backward_rows_group_shift(nch);
        const int grid = ceil_div((int64_t)count << shift, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            rows_backward_contract_chunk_kernel<decltype(D1)::value><<<grid, kBlock, 0, stream>>>(
                pos, prow, evid, ew, n, d1, count, v4, nch, shift, rden, d_b, x, nrhs, d, d_grad_x, d_filtered);
        });
    } else {
        L->kn_rows_slice = "rows_backward_contract_wide_kernel";
        const int grid = ceil_div(count, kBlock / 64);
        const size_t lds = (size_t)(kBlock / 64) * nch * sizeof(float4);       // <= 64 KiB: nch <= kBackwardRowsMaxCols / 4
        dispatch_d1(d1, [&](auto D1) {
            rows_backward_contract_wide_kernel<decltype(D1)::value><<<grid, kBlock, lds, stream>>>(
                pos, prow, evid, ew, n, d1, count, v4, nch, rden, d_b, x, nrhs, d, d_grad_x, d_filtered);
        });
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
