// plx_query_kernels.h -- slices of a vertex array at located queries (plx_slice_at / plx_slice_at_f64, include/plx.h): one
// templated source, instantiated for float in plx_query.hip and for double in plx_query_f64.hip.  The entry points and
// their argument checks are in plx_api.hip; the kernel that locates the queries (plx_locate) is locate_kernel in
// plx_build.hip, next to the embedding it shares its code with.
//
//   out[q][c] = sum over the corners r = 0..d of query q with vid[r][q] >= 0 of  w[r][q] * values[vid[r][q]][c],
//
// divided by 1 + 2^-d the way the existing slices divide: in fp32 every term is (w g) rounded, then one fused multiply-add
// with the rounded reciprocal (rows_term); in double the sum is divided once.  (vid, w) have the SoA layout of the build's
// evid / ew with nq in place of n, so the sums are those of the row-range slices, Gather<T> (plx_kernels.h), with SKIP =
// true: for a query all of whose corners exist, the same terms in the same order as plx_slice_rows / plx_slice_f64 give the
// same bits.  An absent corner is skipped, never multiplied by zero: the vertex array may hold non-finite values elsewhere.
//
// The three shapes of the row-range slices, chosen by the row width alone:
//   slice_at_v1_kernel     vd = 1: one thread per query;
//   slice_at_chunk_kernel  1..64 chunks of 16 bytes per row: a group of 2^k >= chunks lanes per query, one lane per chunk,
//                          d + 1 compiled in up to kGatherMaxD1, the vector store where the output rows are aligned;
//   slice_at_wide_kernel   more than 64 chunks: one wave per query, its lanes stride over the chunks.
// Output rows are dense [nq][vd] in query order; every element is written by one thread from a sum in a fixed order.
#pragma once

#include "plx_kernels.h"

namespace plx {

template <typename T, int D1>
__global__ __launch_bounds__(kBlock) void slice_at_v1_kernel(const int *__restrict__ vid, const float *__restrict__ w, int64_t nq,
                                                             int d1, const T *__restrict__ values,
                                                             typename Gather<T>::Den den, T *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= nq) return;
    out[q] = Gather<T>::template v1<D1, true>(vid, w, (int)nq, (int)q, d1, values, den);
}

template <typename T, bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void slice_at_chunk_kernel(const int *__restrict__ vid, const float *__restrict__ w,
                                                                int64_t nq, int d1,
                                                                const typename Gather<T>::Vec *__restrict__ values, int vd,
                                                                int nch, int shift, typename Gather<T>::Den den,
                                                                T *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (q >= nq || ch >= nch) return;
    Gather<T>::template store<VEC>(out, (size_t)q, vd, ch,
                                   Gather<T>::template chunk<D1, true>(vid, w, (int)nq, (int)q, d1, values, nch, ch, den));
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void slice_at_wide_kernel(const int *__restrict__ vid, const float *__restrict__ w,
                                                               int64_t nq, int d1,
                                                               const typename Gather<T>::Vec *__restrict__ values, int vd,
                                                               int nch, typename Gather<T>::Den den, T *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        Gather<T>::template store<VEC>(out, (size_t)q, vd, ch,
                                       Gather<T>::template wide<true>(vid, w, (int)nq, (int)q, d1, values, nch, ch, den));
}

// Arguments checked by the entry points (plx_api.hip: nq * stride and m * stride below 2^31, so nq is an int and the grids fit).
template <typename T>
int slice_at_impl(plx_lattice *L, const T *d_values, int vd, const int32_t *d_vid, const float *d_w, int64_t nq, T *d_out,
                  hipStream_t stream)
{
    using Q = Gather<T>;
    using Vec = typename Q::Vec;
    const int d1 = L->d + 1, nch = Q::stride(vd) / Q::kPer;
    const typename Q::Den den = Q::den(L);
    const bool vec = Q::vec_ok(d_out, vd);
    const Vec *vv = reinterpret_cast<const Vec *>(d_values);
    if (vd == 1) {
        L->kn_slice_at = "slice_at_v1_kernel";
        const int grid = ceil_div(nq, kBlock);
        if constexpr (Q::kV1Compiled) {
            dispatch_d1(d1, [&](auto D1) {
                slice_at_v1_kernel<T, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(d_vid, d_w, nq, d1, d_values, den, d_out);
            });
        } else {
            slice_at_v1_kernel<T, 0><<<grid, kBlock, 0, stream>>>(d_vid, d_w, nq, d1, d_values, den, d_out);
        }
    } else if (nch <= kChunkGroupMax) {
        L->kn_slice_at = "slice_at_chunk_kernel";
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div(nq << shift, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            if (vec)
                slice_at_chunk_kernel<T, true, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(d_vid, d_w, nq, d1, vv, vd, nch,
                                                                                                 shift, den, d_out);
            else
                slice_at_chunk_kernel<T, false, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(d_vid, d_w, nq, d1, vv, vd, nch,
                                                                                                  shift, den, d_out);
        });
    } else {
        L->kn_slice_at = "slice_at_wide_kernel";
        const int grid = ceil_div(nq, kBlock / 64);
        if (vec) slice_at_wide_kernel<T, true><<<grid, kBlock, 0, stream>>>(d_vid, d_w, nq, d1, vv, vd, nch, den, d_out);
        else slice_at_wide_kernel<T, false><<<grid, kBlock, 0, stream>>>(d_vid, d_w, nq, d1, vv, vd, nch, den, d_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

// ---- the corner dots of the position gradient (plx_slice_at_dots / plx_slice_at_dots_f64) ---------------------------------
//
//   t[r][q] = <g[q][:], values[vid[r][q]][:]> / (1 + 2^-d)   for the corners found, exactly 0 for the absent ones,
//
// SoA [d + 1][nq] as vid and w.  slice_at is linear in the weights, so t[r][q] is the derivative of <g[q], out[q]> with
// respect to w[r][q]; locate_pullback_kernel (plx_build.hip) takes it through the embedding to the position.  The same three
// shapes as the slices, by the row width alone.  A chunk's columns past vd are stride padding: g (dense [nq][vd]) is not
// read there, and the padding of the vertex row is replaced by zero before the product (it may hold anything, NaN too).
// Every sum runs in a fixed order -- the columns of a chunk in turn, the chunks of a lane in turn, then the xor butterfly
// over the lanes (a + b = b + a: every lane of it ends with the same bits) -- so two calls are bit-equal.  No atomics.
template <typename T> struct QueryDots;

template <> struct QueryDots<float> {
    static __device__ __forceinline__ float4 zero() { return f4_zero(); }
    // acc + the products of the first min(left, 4) columns of the chunk
    static __device__ __forceinline__ float dot(float acc, float4 g, float4 v, int left)
    {
        acc += g.x * v.x;
        if (left > 1) acc += g.y * v.y;
        if (left > 2) acc += g.z * v.z;
        if (left > 3) acc += g.w * v.w;
        return acc;
    }
    static __device__ __forceinline__ float finish(float sum, float rden) { return sum * rden; }
};

template <> struct QueryDots<double> {
    static __device__ __forceinline__ double2 zero() { return VecOps<double2>::zero(); }
    static __device__ __forceinline__ double dot(double acc, double2 g, double2 v, int left)
    {
        acc += g.x * v.x;
        if (left > 1) acc += g.y * v.y;
        return acc;
    }
    static __device__ __forceinline__ double finish(double sum, double denom) { return sum / denom; }
};

template <typename T>
__global__ __launch_bounds__(kBlock) void slice_at_dots_v1_kernel(const int *__restrict__ vid, int64_t nq, int d1,
                                                                  const T *__restrict__ values,
                                                                  typename Gather<T>::Den den, const T *__restrict__ g,
                                                                  T *__restrict__ t)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= nq) return;
    const T gq = g[q];
    for (int r = 0; r < d1; ++r) {
        const int v = vid[(size_t)r * nq + q];
        t[(size_t)r * nq + q] = v >= 0 ? QueryDots<T>::finish(gq * values[v], den) : (T)0;
    }
}

// A group of 2^shift >= nch lanes per query, one chunk per lane.  A lane past the last query or past the last chunk stays
// for the shuffles with a zero partial and no load: its group's other lanes, or the other groups of its wave, need it there.
template <typename T, bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void slice_at_dots_chunk_kernel(const int *__restrict__ vid, int64_t nq, int d1,
                                                                     const typename Gather<T>::Vec *__restrict__ values,
                                                                     int vd, int nch, int shift,
                                                                     typename Gather<T>::Den den, const T *__restrict__ g,
                                                                     T *__restrict__ t)
{
    using Q = Gather<T>;
    using Dt = QueryDots<T>;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = tid >> shift;
    const int ch = (int)(tid & ((1 << shift) - 1));
    const bool live = q < nq && ch < nch;
    const int left = vd - Q::kPer * ch;
    const typename Q::Vec gc = live ? Q::template load<VEC>(g, (size_t)q, vd, ch) : Dt::zero();
    if constexpr (D1 > 0) {
        int v[D1];
        typename Q::Vec gath[D1];
        T part[D1];
#pragma unroll
        for (int r = 0; r < D1; ++r) v[r] = live ? vid[(size_t)r * nq + q] : -1;
#pragma unroll
        for (int r = 0; r < D1; ++r) gath[r] = v[r] >= 0 ? values[(size_t)v[r] * nch + ch] : Dt::zero();
#pragma unroll
        for (int r = 0; r < D1; ++r) part[r] = v[r] >= 0 ? Dt::dot((T)0, gc, gath[r], left) : (T)0;
#pragma unroll
        for (int r = 0; r < D1; ++r)
            for (int o = 1; o < (1 << shift); o <<= 1) part[r] += __shfl_xor(part[r], o);
        if (live && ch == 0) {
#pragma unroll
            for (int r = 0; r < D1; ++r) t[(size_t)r * nq + q] = Dt::finish(part[r], den);
        }
    } else {
        for (int r = 0; r < d1; ++r) {
            const int v = live ? vid[(size_t)r * nq + q] : -1;
            T part = v >= 0 ? Dt::dot((T)0, gc, values[(size_t)v * nch + ch], left) : (T)0;
            for (int o = 1; o < (1 << shift); o <<= 1) part += __shfl_xor(part, o);
            if (live && ch == 0) t[(size_t)r * nq + q] = Dt::finish(part, den);
        }
    }
}

// One wave per query (q is the same in all 64 lanes, so the early return takes whole waves); its lanes stride over the chunks.
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void slice_at_dots_wide_kernel(const int *__restrict__ vid, int64_t nq, int d1,
                                                                    const typename Gather<T>::Vec *__restrict__ values,
                                                                    int vd, int nch, typename Gather<T>::Den den,
                                                                    const T *__restrict__ g, T *__restrict__ t)
{
    using Q = Gather<T>;
    using Dt = QueryDots<T>;
    const int64_t q = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < d1; ++r) {
        const int v = vid[(size_t)r * nq + q];
        if (v < 0) {                                        // the same in every lane
            if (lane == 0) t[(size_t)r * nq + q] = (T)0;
            continue;
        }
        T part = (T)0;
        for (int ch = lane; ch < nch; ch += 64)
            part = Dt::dot(part, Q::template load<VEC>(g, (size_t)q, vd, ch), values[(size_t)v * nch + ch], vd - Q::kPer * ch);
        for (int o = 1; o < 64; o <<= 1) part += __shfl_xor(part, o);
        if (lane == 0) t[(size_t)r * nq + q] = Dt::finish(part, den);
    }
}

// Arguments checked by the entry points (plx_api.hip), as for slice_at_impl.
template <typename T>
int slice_at_dots_impl(plx_lattice *L, const T *d_values, int vd, const int32_t *d_vid, const T *d_gout, int64_t nq, T *d_t,
                       hipStream_t stream)
{
    using Q = Gather<T>;
    using Vec = typename Q::Vec;
    const int d1 = L->d + 1, nch = Q::stride(vd) / Q::kPer;
    const typename Q::Den den = Q::den(L);
    const bool vec = Q::vec_ok(d_gout, vd);
    const Vec *vv = reinterpret_cast<const Vec *>(d_values);
    if (vd == 1) {
        L->kn_dots = "slice_at_dots_v1_kernel";
        slice_at_dots_v1_kernel<T><<<ceil_div(nq, kBlock), kBlock, 0, stream>>>(d_vid, nq, d1, d_values, den, d_gout, d_t);
    } else if (nch <= kChunkGroupMax) {
        L->kn_dots = "slice_at_dots_chunk_kernel";
        const int shift = chunk_group_shift(nch);
        const int grid = ceil_div(nq << shift, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            if (vec)
                slice_at_dots_chunk_kernel<T, true, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(d_vid, nq, d1, vv, vd, nch,
                                                                                                      shift, den, d_gout, d_t);
            else
                slice_at_dots_chunk_kernel<T, false, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(d_vid, nq, d1, vv, vd, nch,
                                                                                                       shift, den, d_gout, d_t);
        });
    } else {
        L->kn_dots = "slice_at_dots_wide_kernel";
        const int grid = ceil_div(nq, kBlock / 64);
        if (vec) slice_at_dots_wide_kernel<T, true><<<grid, kBlock, 0, stream>>>(d_vid, nq, d1, vv, vd, nch, den, d_gout, d_t);
        else slice_at_dots_wide_kernel<T, false><<<grid, kBlock, 0, stream>>>(d_vid, nq, d1, vv, vd, nch, den, d_gout, d_t);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
