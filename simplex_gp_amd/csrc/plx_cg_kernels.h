// plx_cg_kernels.h -- the vector work of a conjugate-gradient iteration next to the MVM, in fp32 and in float64: column dots
// of two row-major [n][vd] matrices (vd = 1 + probes is small, n is large), the update X += alpha P, R -= alpha AP with
// |R|^2, and the direction step P = src + beta P of the plain and of the preconditioned iteration (include/plx.h:
// plx_coldot, plx_cg_update, plx_cg_step_update, plx_cg_step_direction, plx_pcg_step_direction and the _f64 calls).  One
// templated source, instantiated by plx_linalg.hip (float) and plx_cg_f64.hip (double): each holds its entry points and
// the explicit instantiations of the launchers plx_internal.h declares, which plx_pcg.hip, plx_pcg_f64.hip and plx_api.hip
// call.  With T = double every array and every operation is in double.
//
// torch's (a*b).sum(0) takes 1.3 ms on [1e6][11] and its CG step is 2 addcmul_ + a column dot = three passes over [n][vd]
// plus a mul_/add_ pair for the direction and ten tiny elementwise launches for "alpha = active ? rs / pAp : 0"; here a dot
// is two streaming reads (~20 us), each step is one pass, and the coefficients are formed on the device from the
// iteration's scalars (no host round trip):
//   update:     alpha = active ? rs / max(pAp, tiny) : 0 (or given);  X += alpha P;  R -= alpha AP;  partial |R|^2
//   direction:  beta = active ? num / max(den, tiny) : 0;  P = src + beta P;  active' = active and sqrt(rr) / b_norm > tol
//               CG: src = R, num = rr = |R'|^2, den = |R|^2 (num and rr are then one read-only pointer);
//               PCG: src = Z, num = <R', Z'>, den = <R, Z>, rr = the true |R'|^2.
// Per-workgroup partial sums through LDS in a fixed order, then one workgroup per column adds the partial rows in a fixed
// order: no atomics, bitwise reproducible.
//
// What the types differ in, all of it in Cg<T>: the guard (1e-30f / 1e-300: a right-hand side scaled by 1e-20 has pAp near
// 1e-40, where the fp32 guard would turn a double alpha into garbage), the 16-byte vector of the direction step (float4 /
// double2) and fmaxf / sqrtf against fmax / sqrt.  What the entry points accept differs too and comes from them (CgRules).
#pragma once
#include "plx_internal.h"

#include <math.h>

namespace plx {

constexpr int kDotBlocks = 1024;      // workgroups of a row stream = rows of partial sums (plx_coldot_work_floats / _doubles)
constexpr int kFinalBlock = 1024;

// kLanes, Vec, guard(), root()
template <class T> struct Cg;
template <> struct Cg<float> {
    static constexpr int kLanes = 4;
    using Vec = float4;
    static __device__ __forceinline__ float guard(float x) { return fmaxf(x, 1e-30f); }
    static __device__ __forceinline__ float root(float x) { return sqrtf(x); }
};
template <> struct Cg<double> {
    static constexpr int kLanes = 2;
    using Vec = double2;
    static __device__ __forceinline__ double guard(double x) { return fmax(x, 1e-300); }
    static __device__ __forceinline__ double root(double x) { return sqrt(x); }
};

// alpha and beta of column c: active ? num / max(den, tiny) : 0
template <class T>
__device__ __forceinline__ T cg_coef(const T *num, const T *den, const T *active, int c)
{
    return active[c] > T(0) ? num[c] / Cg<T>::guard(den[c]) : T(0);
}

// ---- the row-lane stream --------------------------------------------------------------------------------------------------
// threads = (row lane, column lane), column fastest, cw = vd lanes per row: a workgroup step covers kBlock / vd whole rows,
// i.e. consecutive threads read consecutive elements -- a 64-lane wave covers consecutive bytes whatever vd is (with a
// power-of-two lane count per row, 5 of 16 lanes idled at vd = 11 and every fp32 row was its own 44-byte segment:
// cg_step_update 51-55 -> 49 us, 46 us being its streaming floor).  coef(c) is evaluated once by every thread with a
// row lane (the last kBlock % vd threads have none), term(i, coef) once per element i = r vd + c of the thread's rows; the
// terms of a column are added per thread, then over the row lanes through red[kBlock] in a fixed order.
template <class T, class Coef, class Term>
__device__ __forceinline__ void row_lane_stream(T *red, int64_t n, int vd, int cw, T *__restrict__ partial, Coef coef, Term term)
{
    const int c = threadIdx.x % cw;
    const int rl = threadIdx.x / cw;
    const int rows_per_step = kBlock / cw;
    const int64_t rows_per_block = (n + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + rows_per_block, n);
    T acc = T(0);
    if (rl < rows_per_step) {
        const T a = coef(c);
        for (int64_t r = r0 + rl; r < r1; r += rows_per_step) acc += term(r * vd + c, a);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0 && c < vd) {
        T s = T(0);
        for (int k = 0; k < rows_per_step; ++k) s += red[k * cw + c];
        partial[(size_t)blockIdx.x * vd + c] = s;
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void coldot_partial_kernel(const T *__restrict__ a, const T *__restrict__ b, int64_t n,
                                                                int vd, int cw, T *__restrict__ partial)
{
    __shared__ T red[kBlock];
    row_lane_stream(red, n, vd, cw, partial, [](int) { return T(0); }, [&](int64_t i, T) { return a[i] * b[i]; });
}

// STEP: alpha formed from the iteration's scalars (coef = rs, den = pAp; workgroup 0 stores it in alpha_out); otherwise
// coef holds alpha itself and den, active and alpha_out are not read
template <class T, bool STEP>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(T *__restrict__ X, T *__restrict__ R, const T *__restrict__ P,
                                                           const T *__restrict__ AP, const T *__restrict__ coef,
                                                           const T *__restrict__ den, const T *__restrict__ active, int64_t n,
                                                           int vd, int cw, T *__restrict__ partial, T *__restrict__ alpha_out)
{
    __shared__ T red[kBlock];
    row_lane_stream(
        red, n, vd, cw, partial,
        [&](int c) {
            if constexpr (!STEP) return coef[c];
            else {
                const T a = cg_coef(coef, den, active, c);
                if (blockIdx.x == 0 && threadIdx.x < (unsigned)cw) alpha_out[c] = a;      // (row lane 0)
                return a;
            }
        },
        [&](int64_t i, T a) {
            X[i] += P[i] * a;
            const T res = R[i] - AP[i] * a;
            R[i] = res;
            return res * res;
        });
}

// ---- the final column sum -------------------------------------------------------------------------------------------------
// One workgroup per column over `nrows` partial rows of `stride` elements; 1024 threads with four independent loads in
// flight each (the partials of the fused slice + dot are one row per 256-thread tile: 11,719 rows at N = 1e6, vd = 12 -- 256
// threads with one load in flight took 11 us, twice per CG iteration).  Fixed summation order: thread-strided partial sums,
// then a tree.
template <class T>
__global__ __launch_bounds__(kFinalBlock) void coldot_final_kernel(const T *__restrict__ partial, int nrows, int stride,
                                                                   T *__restrict__ out)
{
    __shared__ T red[kFinalBlock];
    const int c = blockIdx.x;
    T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
    int k = threadIdx.x;
    for (; k + 3 * kFinalBlock < nrows; k += 4 * kFinalBlock) {
        const T p0 = partial[(size_t)k * stride + c], p1 = partial[(size_t)(k + kFinalBlock) * stride + c];
        const T p2 = partial[(size_t)(k + 2 * kFinalBlock) * stride + c], p3 = partial[(size_t)(k + 3 * kFinalBlock) * stride + c];
        a0 += p0; a1 += p1; a2 += p2; a3 += p3;
    }
    for (; k < nrows; k += kFinalBlock) a0 += partial[(size_t)k * stride + c];
    red[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    for (int s = kFinalBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = red[0];
}

// ---- the direction step ---------------------------------------------------------------------------------------------------
// workgroup 0 stores the step's scalars
template <class T>
__device__ __forceinline__ void direction_scalars(const T *num, const T *den, const T *rr, const T *active, const T *b_norm,
                                                  T tol, int vd, T *beta_out, T *active_out)
{
    if (blockIdx.x == 0 && (int)threadIdx.x < vd) {
        const int c = threadIdx.x;
        beta_out[c] = cg_coef(num, den, active, c);
        active_out[c] = (active[c] > T(0) && Cg<T>::root(rr[c]) / b_norm[c] > tol) ? T(1) : T(0);
    }
}

// beta per column once per workgroup; the column of element i = blockIdx * kBlock + tid from 32-bit residues (a 64-bit
// i % vd per element costs more than the update itself)
template <class T>
__global__ __launch_bounds__(kBlock) void step_direction_kernel(T *__restrict__ P, const T *__restrict__ src,
                                                                const T *__restrict__ num, const T *__restrict__ den,
                                                                const T *__restrict__ rr, const T *__restrict__ active,
                                                                const T *__restrict__ b_norm, T tol, int64_t total, int vd,
                                                                T *__restrict__ beta_out, T *__restrict__ active_out)
{
    __shared__ T sbeta[kBlock];
    if ((int)threadIdx.x < vd) sbeta[threadIdx.x] = cg_coef(num, den, active, threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < total) {
        const uint32_t uvd = (uint32_t)vd;
        const uint32_t bm = ((blockIdx.x % uvd) * ((uint32_t)kBlock % uvd)) % uvd;      // wave-uniform
        const uint32_t c = (bm + threadIdx.x) % uvd;
        P[i] = src[i] + P[i] * sbeta[c];
    }
    direction_scalars(num, den, rr, active, b_norm, tol, vd, beta_out, active_out);
}

// the same, one 16-byte vector of L = Cg<T>::kLanes elements per thread (total a multiple of L, P and src 16-byte aligned)
template <class T>
__global__ __launch_bounds__(kBlock) void step_direction_vec_kernel(typename Cg<T>::Vec *__restrict__ P,
                                                                    const typename Cg<T>::Vec *__restrict__ src,
                                                                    const T *__restrict__ num, const T *__restrict__ den,
                                                                    const T *__restrict__ rr, const T *__restrict__ active,
                                                                    const T *__restrict__ b_norm, T tol, int64_t vecs, int vd,
                                                                    T *__restrict__ beta_out, T *__restrict__ active_out)
{
    constexpr uint32_t L = Cg<T>::kLanes;
    __shared__ T sbeta[kBlock];
    if ((int)threadIdx.x < vd) sbeta[threadIdx.x] = cg_coef(num, den, active, threadIdx.x);
    __syncthreads();
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q < vecs) {
        const uint32_t uvd = (uint32_t)vd;
        // column of element L q = L (blockIdx kBlock + tid) mod vd, from 32-bit residues
        const uint32_t bm = ((blockIdx.x % uvd) * ((L * (uint32_t)kBlock) % uvd)) % uvd;      // wave-uniform
        uint32_t c = (bm + L * threadIdx.x) % uvd;
        const typename Cg<T>::Vec r = src[q];
        typename Cg<T>::Vec p = P[q];
        const T *re = reinterpret_cast<const T *>(&r);
        T *pe = reinterpret_cast<T *>(&p);
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            pe[j] = re[j] + pe[j] * sbeta[c];
            if (j + 1 < L) c = c + 1 == uvd ? 0 : c + 1;
        }
        P[q] = p;
    }
    direction_scalars(num, den, rr, active, b_norm, tol, vd, beta_out, active_out);
}

// ---- launch side ----------------------------------------------------------------------------------------------------------
template <class T>
int coldot_final(const T *d_partial, int nrows, int stride, int vd, T *d_out, hipStream_t stream)
{
    coldot_final_kernel<T><<<vd, kFinalBlock, 0, stream>>>(d_partial, nrows, stride, d_out);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <class T>
int cg_coldot(const CgRules &rules, const T *d_a, const T *d_b, int64_t n, int vd, T *d_out, T *d_work, hipStream_t s)
{
    PLX_TRY(cg_check(rules, {d_a, d_b, d_out, d_work}, n, vd));
    coldot_partial_kernel<T><<<kDotBlocks, kBlock, 0, s>>>(d_a, d_b, n, vd, vd, d_work);      // cw = vd lanes per row
    return coldot_final(d_work, kDotBlocks, vd, vd, d_out, s);
}

template <class T>
int cg_update(const CgRules &rules, T *d_x, T *d_r, const T *d_p, const T *d_ap, const T *d_alpha, int64_t n, int vd,
              T *d_rs_new, T *d_work, hipStream_t s)
{
    PLX_TRY(cg_check(rules, {d_x, d_r, d_p, d_ap, d_alpha, d_rs_new, d_work}, n, vd));
    cg_update_kernel<T, false><<<kDotBlocks, kBlock, 0, s>>>(d_x, d_r, d_p, d_ap, d_alpha, nullptr, nullptr, n, vd, vd, d_work, nullptr);
    return coldot_final(d_work, kDotBlocks, vd, vd, d_rs_new, s);
}

template <class T>
int cg_step_update(const CgRules &rules, T *d_x, T *d_r, const T *d_p, const T *d_ap, const T *d_rs, const T *d_pap,
                   const T *d_active, int64_t n, int vd, T *d_rs_new, T *d_alpha, T *d_work, hipStream_t s)
{
    PLX_TRY(cg_check(rules, {d_x, d_r, d_p, d_ap, d_rs, d_pap, d_active, d_rs_new, d_alpha, d_work}, n, vd));
    cg_update_kernel<T, true><<<kDotBlocks, kBlock, 0, s>>>(d_x, d_r, d_p, d_ap, d_rs, d_pap, d_active, n, vd, vd, d_work, d_alpha);
    return coldot_final(d_work, kDotBlocks, vd, vd, d_rs_new, s);
}

template <class T>
int cg_step_direction(const CgRules &rules, T *d_p, const T *d_src, const T *d_num, const T *d_den, const T *d_rr,
                      const T *d_active, const T *d_b_norm, T tol, int64_t n, int vd, T *d_beta, T *d_active_out,
                      hipStream_t s)
{
    using Vec = typename Cg<T>::Vec;
    PLX_TRY(cg_check(rules, {d_p, d_src, d_num, d_den, d_rr, d_active, d_b_norm, d_beta, d_active_out}, n, vd,
                     d_active == d_active_out));
    const int64_t total = n * vd;
    if (total > 0 && total % Cg<T>::kLanes == 0 && ((reinterpret_cast<uintptr_t>(d_p) | reinterpret_cast<uintptr_t>(d_src)) & 15) == 0) {
        const int64_t vecs = total / Cg<T>::kLanes;
        step_direction_vec_kernel<T><<<ceil_div(vecs, kBlock), kBlock, 0, s>>>(
            reinterpret_cast<Vec *>(d_p), reinterpret_cast<const Vec *>(d_src), d_num, d_den, d_rr, d_active, d_b_norm, tol, vecs,
            vd, d_beta, d_active_out);
    } else {
        const int grid = total > 0 ? ceil_div(total, kBlock) : 1;      // (n = 0: workgroup 0 still stores the scalars)
        step_direction_kernel<T><<<grid, kBlock, 0, s>>>(d_p, d_src, d_num, d_den, d_rr, d_active, d_b_norm, tol, total, vd,
                                                         d_beta, d_active_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

// the two launchers other translation units call (plx_internal.h), for the one that holds the kernels of T
#define PLX_CG_INSTANTIATE(T)                                                                                                  \
    template int coldot_final<T>(const T *, int, int, int, T *, hipStream_t);                                                   \
    template int cg_step_direction<T>(const CgRules &, T *, const T *, const T *, const T *, const T *, const T *, const T *, T, \
                                      int64_t, int, T *, T *, hipStream_t);

}  // namespace plx
