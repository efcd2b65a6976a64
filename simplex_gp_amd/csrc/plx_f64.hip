// plx_f64.hip -- the float64 product on a built lattice: plx_splat_f64 / plx_blur_f64 / plx_slice_f64 / plx_apply_f64
// (include/plx.h; the entry points and their argument checks are in plx_api.hip).
//
// The operator is the fp32 one's structure carried in double: the vertex ids, the fp32 barycentric weights, the neighbour
// table and the fp32 taps of the build, each converted exactly to double, every sum in double, the result divided by
// 1 + 2^-d in double.  Nothing here reads or writes what the fp32 kernels use per MVM; the tables are the build's (evid / ew,
// nbr, the point permutation) plus ensure_csr's vertex-sorted corners and their row pointer.
//
// Value rows: vd = 1 -> one double per vertex; vd > 1 -> vdp = vd rounded up to 2 doubles, i.e. nch = vdp / 2 double2
// "chunks", one aligned 16-byte access per lane.  Rows of d_src / d_out are in the caller's order, always.
//
// Kernels (256-thread workgroups, wave64), the three shapes of plx_rows_kernels.h per gather stage:
//   f64_splat_v1_kernel     vd = 1: one thread per vertex adds up its corners, in ensure_csr's order;
//   f64_splat_chunk_kernel  1..64 chunks per row: a group of G = 2^k >= chunks lanes per vertex, one lane per chunk;
//   f64_splat_wide_kernel   more than 64 chunks: one wave per vertex, its lanes stride over the chunks;
//   f64_blur_v1_kernel / f64_blur_chunk_kernel  one launch per axis, one thread per (vertex, chunk); the order compiled in
//                           for 0..3 (all neighbour ids, then all gathers, in flight at once), a run-time loop above that;
//   f64_slice_v1_kernel / f64_slice_chunk_kernel / f64_slice_wide_kernel  one thread (group, wave) per point in LATTICE
//                           order -- entry tables read in streams, neighbouring points gather the same vertex rows -- the
//                           result stored to the caller's row through the point permutation.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, bitwise reproducible.

#include "plx_kernels.h"

#include <math.h>

#include <utility>

namespace plx {

// ---- splat (f64_load_chunk / f64_store_chunk / f64_vertex_sum / f64_point_sum: plx_kernels.h) ----------------------------
__global__ __launch_bounds__(kBlock) void f64_splat_v1_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                              const float *__restrict__ w, const double *__restrict__ src,
                                                              int m, double *__restrict__ values)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    double acc = 0.0;
    for (int j = ptr[v], j1 = ptr[v + 1]; j < j1; ++j) acc += (double)w[j] * src[row[j] & 0x7FFFFFFF];
    values[v] = acc;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void f64_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                 const float *__restrict__ w, const double *__restrict__ src,
                                                                 int vd, int nch, int shift, int m,
                                                                 double2 *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = f64_vertex_sum<VEC>(row, w, ptr[v], ptr[v + 1], src, vd, ch);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void f64_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                const float *__restrict__ w, const double *__restrict__ src,
                                                                int vd, int nch, int m, double2 *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = f64_vertex_sum<VEC>(row, w, j0, j1, src, vd, ch);
}

// ---- blur ----------------------------------------------------------------------------------------------------------
// One axis: out[v] = c[r] old[v] + sum_s c[tap of slot s] old[nbr[s][v]], slots -r..-1, 1..r as the build lays them out,
// absent neighbours (-1) contributing nothing.  V = double (vd = 1) or double2 (rowlen chunks per vertex).
// ORDER >= 0: compiled in; -1: order_rt.
template <class V, int ORDER>
__device__ __forceinline__ void f64_blur_item(const V *__restrict__ old, V *__restrict__ out, const int *__restrict__ nbr,
                                              int m, int64_t mstride, int rowlen, int order_rt, const double *c, int ntiles)
{
    using O = VecOps<V>;
    const int tile = tile_index(ntiles);
    if (tile < 0) return;
    const uint32_t item = (uint32_t)tile * kBlock + threadIdx.x;      // (the entry point checks m * rowlen < 2^31)
    if (item >= (uint32_t)m * (uint32_t)rowlen) return;
    const uint32_t i = item / (uint32_t)rowlen, ch = item - i * (uint32_t)rowlen;
    V acc = O::zero();
    if constexpr (ORDER >= 0) {
        int id[2 * ORDER + 1];
        V g[2 * ORDER + 1];
#pragma unroll
        for (int s = 0; s < 2 * ORDER; ++s) id[s] = nbr[s * mstride + i];
#pragma unroll
        for (int s = 0; s < 2 * ORDER; ++s) g[s] = old[id[s] >= 0 ? (size_t)id[s] * rowlen + ch : (size_t)item];
        const V centre = old[item];
#pragma unroll
        for (int s = 0; s < ORDER; ++s)
            if (id[s] >= 0) O::fma(acc, c[s], g[s]);
        O::fma(acc, c[ORDER], centre);
#pragma unroll
        for (int s = 0; s < ORDER; ++s)
            if (id[ORDER + s] >= 0) O::fma(acc, c[ORDER + 1 + s], g[ORDER + s]);
    } else {
        const int order = order_rt;
        for (int s = 0; s < order; ++s) {
            const int nb = nbr[s * mstride + i];
            if (nb >= 0) O::fma(acc, c[s], old[(size_t)nb * rowlen + ch]);
        }
        O::fma(acc, c[order], old[item]);
        for (int s = 0; s < order; ++s) {
            const int nb = nbr[(order + s) * mstride + i];
            if (nb >= 0) O::fma(acc, c[order + 1 + s], old[(size_t)nb * rowlen + ch]);
        }
    }
    out[item] = acc;
}

template <int ORDER>
__global__ __launch_bounds__(kBlock) void f64_blur_v1_kernel(const double *__restrict__ old, double *__restrict__ out,
                                                             const int *__restrict__ nbr, int m, int64_t mstride,
                                                             int order_rt, TapArgs64 taps, int ntiles)
{
    f64_blur_item<double, ORDER>(old, out, nbr, m, mstride, 1, order_rt, taps.c, ntiles);
}

template <int ORDER>
__global__ __launch_bounds__(kBlock) void f64_blur_chunk_kernel(const double2 *__restrict__ old, double2 *__restrict__ out,
                                                                const int *__restrict__ nbr, int m, int64_t mstride,
                                                                int rowlen, int order_rt, TapArgs64 taps, int ntiles)
{
    f64_blur_item<double2, ORDER>(old, out, nbr, m, mstride, rowlen, order_rt, taps.c, ntiles);
}

// ---- slice ---------------------------------------------------------------------------------------------------------
// D1 > 0: d + 1 compiled in (all index loads, then all gathers, then the ordered sum); 0: the run-time form.  The chunk sum
// is f64_filtered_chunk (plx_kernels.h), shared with the row-range and the query slices; the vd = 1 sum is f64_filtered_v1
// there, written out here because the call moved two instructions of the run-time loop.
template <int D1>
__global__ __launch_bounds__(kBlock) void f64_slice_v1_kernel(const uint32_t *__restrict__ perm, const int *__restrict__ evid,
                                                              const float *__restrict__ ew, int n, int d1,
                                                              const double *__restrict__ values, double denom,
                                                              double *__restrict__ out)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
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
    out[perm[p]] = acc / denom;
}

template <bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void f64_slice_chunk_kernel(const uint32_t *__restrict__ perm,
                                                                 const int *__restrict__ evid, const float *__restrict__ ew,
                                                                 int n, int d1, const double2 *__restrict__ values, int vd,
                                                                 int nch, int shift, double denom, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t p64 = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (p64 >= n || ch >= nch) return;
    const int p = (int)p64;
    const double2 acc = f64_filtered_chunk<D1>(evid, ew, n, p, d1, values, nch, ch, denom);
    f64_store_chunk<VEC>(out, (size_t)perm[p], vd, ch, acc);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void f64_slice_wide_kernel(const uint32_t *__restrict__ perm,
                                                                const int *__restrict__ evid, const float *__restrict__ ew,
                                                                int n, int d1, const double2 *__restrict__ values, int vd,
                                                                int nch, double denom, double *__restrict__ out)
{
    const int64_t p64 = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (p64 >= n) return;
    const int p = (int)p64;
    const size_t row = (size_t)perm[p];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        f64_store_chunk<VEC>(out, row, vd, ch, f64_point_sum(evid, ew, n, p, d1, values, nch, ch, denom));
}

// ---- launch side (kChunkGroupMax / f64_vec_ok / chunk_group_shift: plx_kernels.h) -----------------------------------------------
// The vertex-sorted corners of the current build and the first corner of every vertex (ensure_csr + its row pointer):
// built by the first fp64 splat after a build, kept until the next one.
static int ensure_f64_tables(plx_lattice *L, hipStream_t stream)
{
    if (L->f64_gen == L->build_gen) return PLX_OK;
    PLX_TRY(refuse_under_capture(stream, "the vertex row pointer of the float64 splat"));
    PLX_TRY(export_row_ptr(L, stream));
    L->f64_gen = L->build_gen;
    return PLX_OK;
}

int splat_f64_impl(plx_lattice *L, const double *d_src, int vd, double *d_values, hipStream_t stream)
{
    PLX_TRY(ensure_f64_tables(L, stream));
    const int m = (int)L->m, nch = values_stride_f64(vd) / 2;
    const int *ptr = L->row_ptr.as<int>(), *row = L->csr_row.as<int>();
    const float *w = L->csr_w.as<float>();
    const bool vec = f64_vec_ok(d_src, vd);
    double2 *v2 = reinterpret_cast<double2 *>(d_values);
    if (vd == 1) {
        L->kn_f64_splat = "f64_splat_v1_kernel";
        f64_splat_v1_kernel<<<ceil_div(m, kBlock), kBlock, 0, stream>>>(ptr, row, w, d_src, m, d_values);
    } else if (nch <= kChunkGroupMax) {
        L->kn_f64_splat = "f64_splat_chunk_kernel";
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        if (vec) f64_splat_chunk_kernel<true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, v2);
        else f64_splat_chunk_kernel<false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, v2);
    } else {
        L->kn_f64_splat = "f64_splat_wide_kernel";
        const int grid = ceil_div(m, kBlock / 64);
        if (vec) f64_splat_wide_kernel<true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, v2);
        else f64_splat_wide_kernel<false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, v2);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <int ORDER>
static void launch_blur_f64(plx_lattice *L, const double *old, double *out, const int *nbr, int vd, const TapArgs64 &taps,
                            hipStream_t stream)
{
    const int m = (int)L->m, rowlen = vd == 1 ? 1 : values_stride_f64(vd) / 2;
    const int ntiles = ceil_div((int64_t)m * rowlen, kBlock);
    if (vd == 1)
        f64_blur_v1_kernel<ORDER><<<tile_grid(ntiles), kBlock, 0, stream>>>(old, out, nbr, m, L->mstride, L->order, taps, ntiles);
    else
        f64_blur_chunk_kernel<ORDER><<<tile_grid(ntiles), kBlock, 0, stream>>>(
            reinterpret_cast<const double2 *>(old), reinterpret_cast<double2 *>(out), nbr, m, L->mstride, rowlen, L->order, taps,
            ntiles);
}

void blur_axis_f64(plx_lattice *L, const double *old, double *out, int axis, int vd, const TapArgs64 &taps, hipStream_t stream)
{
    const int order = L->order;
    const int *nbr = L->nbr.as<int>() + (size_t)axis * 2 * order * L->mstride;
    L->kn_f64_blur = vd == 1 ? "f64_blur_v1_kernel" : "f64_blur_chunk_kernel";
    switch (order) {
    case 0: launch_blur_f64<0>(L, old, out, nbr, vd, taps, stream); break;
    case 1: launch_blur_f64<1>(L, old, out, nbr, vd, taps, stream); break;
    case 2: launch_blur_f64<2>(L, old, out, nbr, vd, taps, stream); break;
    case 3: launch_blur_f64<3>(L, old, out, nbr, vd, taps, stream); break;
    default: launch_blur_f64<-1>(L, old, out, nbr, vd, taps, stream); break;
    }
}

int blur_f64_impl(plx_lattice *L, double *d_values, double *d_scratch, int vd, int *result_in_scratch, hipStream_t stream)
{
    const int d1 = L->d + 1;
    TapArgs64 taps;
    for (int i = 0; i < 2 * PLX_MAX_ORDER + 1; ++i) taps.c[i] = (double)L->taps.c[i];
    double *cur = d_values, *nxt = d_scratch;
    for (int a = 0; a < d1; ++a) {
        blur_axis_f64(L, cur, nxt, a, vd, taps, stream);
        std::swap(cur, nxt);
    }
    *result_in_scratch = cur == d_scratch ? 1 : 0;
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <bool VEC>
static void launch_slice_chunk_f64(plx_lattice *L, const double2 *v2, int vd, int nch, double denom, double *d_out,
                                   hipStream_t stream)
{
    const int n = (int)L->n, d1 = L->d + 1;
    const int shift = chunk_group_shift(nch);
    const int grid = ceil_div((int64_t)n << shift, kBlock);
    const uint32_t *perm = L->perm.as<uint32_t>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    dispatch_d1(d1, [&](auto D1) {
        f64_slice_chunk_kernel<VEC, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, v2, vd,
                                                                                      nch, shift, denom, d_out);
    });
}

int slice_f64_impl(plx_lattice *L, const double *d_values, int vd, double *d_out, hipStream_t stream)
{
    const int n = (int)L->n, d1 = L->d + 1, nch = values_stride_f64(vd) / 2;
    const double denom = 1.0 + ldexp(1.0, -L->d);
    const uint32_t *perm = L->perm.as<uint32_t>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const bool vec = f64_vec_ok(d_out, vd);
    const double2 *v2 = reinterpret_cast<const double2 *>(d_values);
    if (vd == 1) {
        L->kn_f64_slice = "f64_slice_v1_kernel";
        const int grid = ceil_div(n, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            f64_slice_v1_kernel<decltype(D1)::value><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, d_values,
                                                                                  denom, d_out);
        });
    } else if (nch <= kChunkGroupMax) {
        L->kn_f64_slice = "f64_slice_chunk_kernel";
        if (vec) launch_slice_chunk_f64<true>(L, v2, vd, nch, denom, d_out, stream);
        else launch_slice_chunk_f64<false>(L, v2, vd, nch, denom, d_out, stream);
    } else {
        L->kn_f64_slice = "f64_slice_wide_kernel";
        const int grid = ceil_div(n, kBlock / 64);
        if (vec) f64_slice_wide_kernel<true><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, v2, vd, nch, denom, d_out);
        else f64_slice_wide_kernel<false><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, v2, vd, nch, denom, d_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
