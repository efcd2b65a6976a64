// plx_query_kernels.h -- slices of a vertex array at located queries (plx_slice_at / plx_slice_at_f64, include/plx.h): one
// templated source, instantiated for float in plx_query.hip and for double in plx_query_f64.hip.  The entry points and
// their argument checks are in plx_api.hip; the kernel that locates the queries (plx_locate) is locate_kernel in
// plx_build.hip, next to the embedding it shares its code with.
//
//   out[q][c] = sum over the corners r = 0..d of query q with vid[r][q] >= 0 of  w[r][q] * values[vid[r][q]][c],
//
// divided by 1 + 2^-d the way the existing slices divide: in fp32 every term is (w g) rounded, then one fused multiply-add
// with the rounded reciprocal (rows_term); in double the sum is divided once.  (vid, w) have the SoA layout of the build's
// evid / ew with nq in place of n, so the sums are the shared helpers of plx_kernels.h -- rows_point_sum /
// rows_filtered_chunk and f64_point_sum -- with their SKIP flag: for a query all of whose corners exist, the same terms in
// the same order as plx_slice_rows / plx_slice_f64 give the same bits.  An absent corner is skipped, never multiplied by
// zero: the vertex array may hold non-finite values elsewhere.
//
// The three shapes of the row-range slices, chosen by the row width alone:
//   slice_at_v1_kernel     vd = 1: one thread per query;
//   slice_at_chunk_kernel  1..64 chunks of 16 bytes per row: a group of 2^k >= chunks lanes per query, one lane per chunk,
//                          d + 1 compiled in up to kGatherMaxD1, the vector store where the output rows are aligned;
//   slice_at_wide_kernel   more than 64 chunks: one wave per query, its lanes stride over the chunks.
// Output rows are dense [nq][vd] in query order; every element is written by one thread from a sum in a fixed order.
#pragma once

#include "plx_kernels.h"

#include <math.h>

namespace plx {

template <typename T> struct QuerySlice;

template <> struct QuerySlice<float> {
    using Vec = float4;                       // one 16-byte chunk of a vertex row
    using Den = float;                        // the rounded reciprocal of 1 + 2^-d
    static constexpr int kPer = 4;            // elements per chunk
    static constexpr bool kV1Compiled = false;      // rows_slice_v1_kernel reads its corners in a run-time loop
    static int stride(int vd) { return values_stride(vd); }
    static Den den(const plx_lattice *L) { return 1.0f / L->slice_denom; }
    static bool vec_ok(const void *p, int vd) { return (vd & 3) == 0 && ((uintptr_t)p & 15) == 0; }
    // the sum of rows_slice_v1_kernel
    template <int D1>
    static __device__ __forceinline__ float v1(const int *__restrict__ vid, const float *__restrict__ w, int nq, int q,
                                               int d1, const float *__restrict__ values, float rden)
    {
        float acc = 0.f;
        for (int r = 0; r < d1; ++r) {
            const int v = vid[(size_t)r * nq + q];
            if (v < 0) continue;
            acc += w[(size_t)r * nq + q] * values[v] * rden;
        }
        return acc;
    }
    template <int D1>
    static __device__ __forceinline__ float4 chunk(const int *__restrict__ vid, const float *__restrict__ w, int nq, int q,
                                                   int d1, const float4 *__restrict__ values, int nch, int ch, float rden)
    {
        return rows_filtered_chunk<D1, true>(vid, w, nq, q, d1, values, nch, ch, rden);
    }
    static __device__ __forceinline__ float4 wide(const int *__restrict__ vid, const float *__restrict__ w, int nq, int q,
                                                  int d1, const float4 *__restrict__ values, int nch, int ch, float rden)
    {
        return rows_point_sum<true>(vid, w, nq, q, d1, values, nch, ch, rden);
    }
    template <bool VEC>
    static __device__ __forceinline__ void store(float *__restrict__ out, size_t row, int vd, int ch, float4 a)
    {
        float *o = out + row * vd + 4 * ch;
        if constexpr (VEC) { *reinterpret_cast<float4 *>(o) = a; return; }
        const int left = vd - 4 * ch;
        o[0] = a.x;
        if (left > 1) o[1] = a.y;
        if (left > 2) o[2] = a.z;
        if (left > 3) o[3] = a.w;
    }
};

template <> struct QuerySlice<double> {
    using Vec = double2;
    using Den = double;                       // 1 + 2^-d itself: the double slices divide
    static constexpr int kPer = 2;
    static constexpr bool kV1Compiled = true;       // f64_slice_v1_kernel has d + 1 compiled in
    static int stride(int vd) { return values_stride_f64(vd); }
    static Den den(const plx_lattice *L) { return 1.0 + ldexp(1.0, -L->d); }
    static bool vec_ok(const void *p, int vd) { return f64_vec_ok(p, vd); }
    // the sum of f64_slice_v1_kernel (D1 > 0: all ids, then all gathers, then the ordered sum)
    template <int D1>
    static __device__ __forceinline__ double v1(const int *__restrict__ vid, const float *__restrict__ w, int nq, int q,
                                                int d1, const double *__restrict__ values, double denom)
    {
        double acc = 0.0;
        if constexpr (D1 > 0) {
            int v[D1];
            double g[D1];
#pragma unroll
            for (int r = 0; r < D1; ++r) v[r] = vid[(size_t)r * nq + q];
#pragma unroll
            for (int r = 0; r < D1; ++r) g[r] = v[r] >= 0 ? values[v[r]] : 0.0;
#pragma unroll
            for (int r = 0; r < D1; ++r)
                if (v[r] >= 0) acc += (double)w[(size_t)r * nq + q] * g[r];
        } else {
            for (int r = 0; r < d1; ++r) {
                const int v = vid[(size_t)r * nq + q];
                if (v < 0) continue;
                acc += (double)w[(size_t)r * nq + q] * values[v];
            }
        }
        return acc / denom;
    }
    // the sum of f64_slice_chunk_kernel
    template <int D1>
    static __device__ __forceinline__ double2 chunk(const int *__restrict__ vid, const float *__restrict__ w, int nq,
                                                    int q, int d1, const double2 *__restrict__ values, int nch, int ch,
                                                    double denom)
    {
        if constexpr (D1 > 0) {
            int v[D1];
            double2 g[D1];
#pragma unroll
            for (int r = 0; r < D1; ++r) v[r] = vid[(size_t)r * nq + q];
#pragma unroll
            for (int r = 0; r < D1; ++r) g[r] = v[r] >= 0 ? values[(size_t)v[r] * nch + ch] : VecOps<double2>::zero();
            double2 acc = VecOps<double2>::zero();
#pragma unroll
            for (int r = 0; r < D1; ++r)
                if (v[r] >= 0) VecOps<double2>::fma(acc, (double)w[(size_t)r * nq + q], g[r]);
            return make_double2(acc.x / denom, acc.y / denom);
        } else {
            return f64_point_sum<true>(vid, w, nq, q, d1, values, nch, ch, denom);
        }
    }
    static __device__ __forceinline__ double2 wide(const int *__restrict__ vid, const float *__restrict__ w, int nq, int q,
                                                   int d1, const double2 *__restrict__ values, int nch, int ch, double denom)
    {
        return f64_point_sum<true>(vid, w, nq, q, d1, values, nch, ch, denom);
    }
    template <bool VEC>
    static __device__ __forceinline__ void store(double *__restrict__ out, size_t row, int vd, int ch, double2 a)
    {
        f64_store_chunk<VEC>(out, row, vd, ch, a);
    }
};

template <typename T, int D1>
__global__ __launch_bounds__(kBlock) void slice_at_v1_kernel(const int *__restrict__ vid, const float *__restrict__ w, int64_t nq,
                                                             int d1, const T *__restrict__ values,
                                                             typename QuerySlice<T>::Den den, T *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= nq) return;
    out[q] = QuerySlice<T>::template v1<D1>(vid, w, (int)nq, (int)q, d1, values, den);
}

template <typename T, bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void slice_at_chunk_kernel(const int *__restrict__ vid, const float *__restrict__ w,
                                                                int64_t nq, int d1,
                                                                const typename QuerySlice<T>::Vec *__restrict__ values, int vd,
                                                                int nch, int shift, typename QuerySlice<T>::Den den,
                                                                T *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (q >= nq || ch >= nch) return;
    QuerySlice<T>::template store<VEC>(out, (size_t)q, vd, ch,
                                       QuerySlice<T>::template chunk<D1>(vid, w, (int)nq, (int)q, d1, values, nch, ch, den));
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void slice_at_wide_kernel(const int *__restrict__ vid, const float *__restrict__ w,
                                                               int64_t nq, int d1,
                                                               const typename QuerySlice<T>::Vec *__restrict__ values, int vd,
                                                               int nch, typename QuerySlice<T>::Den den, T *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        QuerySlice<T>::template store<VEC>(out, (size_t)q, vd, ch, QuerySlice<T>::wide(vid, w, (int)nq, (int)q, d1, values, nch, ch, den));
}

// Arguments checked by the entry points (plx_api.hip: nq * stride and m * stride below 2^31, so nq is an int and the grids fit).
template <typename T>
int slice_at_impl(plx_lattice *L, const T *d_values, int vd, const int32_t *d_vid, const float *d_w, int64_t nq, T *d_out,
                  hipStream_t stream)
{
    using Q = QuerySlice<T>;
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
    template <bool VEC> static __device__ __forceinline__ float4 load(const float *__restrict__ g, size_t row, int vd, int ch)
    {
        const float *p = g + row * vd + 4 * ch;
        if constexpr (VEC) return *reinterpret_cast<const float4 *>(p);
        const int left = vd - 4 * ch;
        return make_float4(p[0], left > 1 ? p[1] : 0.f, left > 2 ? p[2] : 0.f, left > 3 ? p[3] : 0.f);
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
    template <bool VEC> static __device__ __forceinline__ double2 load(const double *__restrict__ g, size_t row, int vd, int ch)
    {
        const double *p = g + row * vd + 2 * ch;
        if constexpr (VEC) return *reinterpret_cast<const double2 *>(p);
        return make_double2(p[0], vd - 2 * ch > 1 ? p[1] : 0.0);
    }
    static __device__ __forceinline__ double finish(double sum, double denom) { return sum / denom; }
};

template <typename T>
__global__ __launch_bounds__(kBlock) void slice_at_dots_v1_kernel(const int *__restrict__ vid, int64_t nq, int d1,
                                                                  const T *__restrict__ values,
                                                                  typename QuerySlice<T>::Den den, const T *__restrict__ g,
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
                                                                     const typename QuerySlice<T>::Vec *__restrict__ values,
                                                                     int vd, int nch, int shift,
                                                                     typename QuerySlice<T>::Den den, const T *__restrict__ g,
                                                                     T *__restrict__ t)
{
    using Q = QuerySlice<T>;
    using Dt = QueryDots<T>;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = tid >> shift;
    const int ch = (int)(tid & ((1 << shift) - 1));
    const bool live = q < nq && ch < nch;
    const int left = vd - Q::kPer * ch;
    const typename Q::Vec gc = live ? Dt::template load<VEC>(g, (size_t)q, vd, ch) : Dt::zero();
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
                                                                    const typename QuerySlice<T>::Vec *__restrict__ values,
                                                                    int vd, int nch, typename QuerySlice<T>::Den den,
                                                                    const T *__restrict__ g, T *__restrict__ t)
{
    using Q = QuerySlice<T>;
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
            part = Dt::dot(part, Dt::template load<VEC>(g, (size_t)q, vd, ch), values[(size_t)v * nch + ch], vd - Q::kPer * ch);
        for (int o = 1; o < 64; o <<= 1) part += __shfl_xor(part, o);
        if (lane == 0) t[(size_t)r * nq + q] = Dt::finish(part, den);
    }
}

// Arguments checked by the entry points (plx_api.hip), as for slice_at_impl.
template <typename T>
int slice_at_dots_impl(plx_lattice *L, const T *d_values, int vd, const int32_t *d_vid, const T *d_gout, int64_t nq, T *d_t,
                       hipStream_t stream)
{
    using Q = QuerySlice<T>;
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
