// plx_exact_kernels.h -- the exact kernel MVM and its position gradient, evaluated on the fly (no N x N matrix is ever
// stored): one templated source for fp32 and for double, instantiated by plx_exact.hip (float) and plx_exact_f64.hip
// (double), two translation units of a few lines each so that the two sets of 225 kernels compile side by side:
//
//   out[i][c]     = sum_j k(|x1_i - x2_j|^2) v[j][c]                                        plx_exact_mvm, plx_exact_mvm_f64
//   grad_x1[i][:] = sum_j 2 k'(|x1_i - x2_j|^2) (x1_i - x2_j) (g_i . v_j)                   plx_exact_grad, plx_exact_grad_f64
//
// k is one of the project's profiles of the squared distance (stencil.py: rbf, matern), compiled in.  This is what the
// lattice stands in for: the yardstick of its approximation error, and the like-for-like speed figure beside it.  With
// T = double every array and every operation is in double and nothing passes through fp32: exp and sqrt are the double
// library functions, the Matern constants round from double literals.  The contract is one: stateless, the caller's
// workspace, no float atomics, every output element written by one thread, graph-capturable.
//
// Layout.  A workgroup of 256 threads owns 256 consecutive rows i, one per thread; x1_i (zero-padded to DP, a multiple
// of 4 >= d) and the row's accumulators stay in registers (a double takes two 32-bit registers).  The j range is walked
// in tiles of ExScalar<T>::kTileJ rows of x2 (and of v, a column block of TC at a time) staged in LDS: 128 rows of
// floats, 64 of doubles -- the same bytes (at most 16 + 8 KiB), and the double tile's sequential sum, the largest term
// of the rounding bound of an entry, is half as long.  Every thread reads the same LDS words (broadcast 16-byte reads of
// four floats or two doubles, no bank conflicts).  Distances are direct differences, sum_k (x1_ik - x2_jk)^2: no norm
// expansion, so no cancellation for close points far from the origin, and d2 >= 0 by construction.  The DP and TC
// ladders serve both types: a padded dimension costs a subtraction and an FMA at the double rate, so the fine DP ladder
// matters more in double, and TC = 16 keeps t = 11 in one column block (the forward recomputes k per block).
//
// Cost model (VALU, per pair and lane): DP subtractions + DP FMAs for d2, the exponential, TC FMAs for the contraction.
// In fp32 the exponential is one v_exp_f32 (8 issue cycles against 4 for an FMA; Matern adds a v_sqrt_f32) and the
// operands come from LDS as broadcast dwordx4 reads.  In double everything runs at the double rate and the exponential
// is software (gfx950 has no double exponential: argument reduction, a degree-11 polynomial and the scaling, counted in
// DESIGN.md section 20), with a Newton square root for the Materns.
//
// Columns: t > TC loops over column blocks; the forward recomputes k per block (its outputs are per block), the gradient
// accumulates over blocks in registers (the gradient is linear in the columns of g and v).
//
// Split j.  When n1 is small (prediction rows, n1 = 8 ...) one workgroup per 256 rows leaves the chip idle, so the j
// range is cut into `splits` slices, each written to its own slab [n1][t or d] of the caller's workspace, and a second
// kernel sums the slabs in slice order.  No float atomics: two identical calls are bitwise equal (plx.h's contract).
// The workspace bound is in bytes and at most 16 MiB, so the cap allows half as many doubles as floats.
#pragma once
#include "plx_internal.h"

#include <algorithm>

namespace plx {

constexpr int kExThreads = 256;                 // rows per workgroup, one per thread
constexpr int64_t kExMaxRows = (int64_t)1 << 31;             // n1, n2 < 2^31
constexpr int64_t kExSplitRowCap = 524288;      // split only while splits * n1 <= this many rows ...
constexpr int64_t kExWorkBytesCap = (int64_t)16 << 20;       // ... and the slabs fit 16 MiB
constexpr int kExMaxSplits = 1024;
constexpr int kExSplitJ = 512;                  // a slice covers at least this many j

// everything that differs between the two scalar types
template <typename T> struct ExScalar;
template <> struct ExScalar<float> {
    static constexpr int kTileJ = 128;                  // x2 / v rows per LDS tile
    static constexpr bool kUnrollForward = true;        // the forward's j loop carries #pragma unroll 2
    static constexpr const char *kWorkBytes = "plx_exact_work_bytes";
    static __device__ __forceinline__ float exp(float x) { return __expf(x); }
    static __device__ __forceinline__ float sqrt(float x) { return sqrtf(x); }
    static __device__ __forceinline__ float fma(float a, float b, float c) { return fmaf(a, b, c); }
};
template <> struct ExScalar<double> {
    static constexpr int kTileJ = 64;
    static constexpr bool kUnrollForward = false;
    static constexpr const char *kWorkBytes = "plx_exact_work_bytes_f64";
    static __device__ __forceinline__ double exp(double x) { return ::exp(x); }
    static __device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
    static __device__ __forceinline__ double fma(double a, double b, double c) { return ::fma(a, b, c); }
};

// the 16-byte LDS read: four floats or two doubles.  A plain struct, not a vector type: with a vector type the compiler
// allocates the gradient kernels' registers differently (profiles/exact_share_measured.md)
template <typename T> constexpr int kExPack = 16 / sizeof(T);
template <typename T> struct alignas(16) ExPack {
    T e[kExPack<T>];
};

template <typename T, int P> struct Profile;

// RBF: k = exp(-d2) (stencil.rbf, the lattice's own RBF -- not GPyTorch's exp(-d2 / 2)); 2 k' = -2 exp(-d2)
template <typename T> struct Profile<T, PLX_PROFILE_RBF> {
    using S = ExScalar<T>;
    static __device__ __forceinline__ T k(T d2) { return S::exp(-d2); }
    static __device__ __forceinline__ T dk2(T d2) { return T(-2) * S::exp(-d2); }
};
// Matern-1/2: k = e^-r; 2 k' = -e^-r / r, singular at r = 0, where the pair contributes 0 (x1_i - x2_j = 0 there)
template <typename T> struct Profile<T, PLX_PROFILE_MATERN12> {
    using S = ExScalar<T>;
    static __device__ __forceinline__ T k(T d2) { return S::exp(-S::sqrt(d2)); }
    static __device__ __forceinline__ T dk2(T d2)
    {
        const T r = S::sqrt(d2);
        return r > T(0) ? -S::exp(-r) / r : T(0);
    }
};
// Matern-3/2: k = (1 + sqrt3 r) e^{-sqrt3 r}; 2 k' = -3 e^{-sqrt3 r}
template <typename T> struct Profile<T, PLX_PROFILE_MATERN32> {
    using S = ExScalar<T>;
    static __device__ __forceinline__ T k(T d2)
    {
        const T s = T(1.7320508075688772) * S::sqrt(d2);
        return (T(1) + s) * S::exp(-s);
    }
    static __device__ __forceinline__ T dk2(T d2) { return T(-3) * S::exp(-T(1.7320508075688772) * S::sqrt(d2)); }
};
// Matern-5/2: k = (1 + sqrt5 r + 5/3 r^2) e^{-sqrt5 r}; 2 k' = -(5/3) (1 + sqrt5 r) e^{-sqrt5 r}
template <typename T> struct Profile<T, PLX_PROFILE_MATERN52> {
    using S = ExScalar<T>;
    static __device__ __forceinline__ T k(T d2)
    {
        const T s = T(2.2360679774997896) * S::sqrt(d2);
        return (T(1) + s + (T(5) / T(3)) * d2) * S::exp(-s);
    }
    static __device__ __forceinline__ T dk2(T d2)
    {
        const T s = T(2.2360679774997896) * S::sqrt(d2);
        return (T(-5) / T(3)) * (T(1) + s) * S::exp(-s);
    }
};

// the workgroup's tile of x2 rows [j0, j0 + jn) into LDS, zero-padded to DP columns; and of column block [c0, c0 + TC)
// of v (zero past t).  Rows past jn are never read.
template <typename T, int DP, int TC>
__device__ __forceinline__ void ex_stage(const T *__restrict__ x2, const T *__restrict__ v, int d, int t, int64_t j0, int jn,
                                         int c0, T *xs, T *vs)
{
    for (int e = threadIdx.x; e < ExScalar<T>::kTileJ * DP; e += kExThreads) {
        const int j = e / DP, k = e % DP;
        xs[e] = (j < jn && k < d) ? x2[(j0 + j) * d + k] : T(0);
    }
    for (int e = threadIdx.x; e < ExScalar<T>::kTileJ * TC; e += kExThreads) {
        const int j = e / TC, c = e % TC;
        vs[e] = (j < jn && c0 + c < t) ? v[(j0 + j) * t + c0 + c] : T(0);
    }
}

// diff = xi - xj and its squared length, a 16-byte read of xj at a time: the subtractions of a read, then its FMAs
template <typename T, int DP>
__device__ __forceinline__ T ex_d2(const T (&xi)[DP], const T *xj, T (&diff)[DP])
{
    T d2 = T(0);
#pragma unroll
    for (int k = 0; k < DP; k += kExPack<T>) {
        const ExPack<T> b = *reinterpret_cast<const ExPack<T> *>(xj + k);
#pragma unroll
        for (int q = 0; q < kExPack<T>; ++q) diff[k + q] = xi[k + q] - b.e[q];
#pragma unroll
        for (int q = 0; q < kExPack<T>; ++q) d2 = ExScalar<T>::fma(diff[k + q], diff[k + q], d2);
    }
    return d2;
}

// the forward's pair (i, j) of a staged tile: tacc[:] += k(d2_ij) v[j][:] (the differences are not kept)
template <typename T, int PROF, int DP, int TC>
__device__ __forceinline__ void ex_mvm_pair(const T (&xi)[DP], const T *xs, const T *vs, int j, T (&tacc)[TC])
{
    T diff[DP];
    const T kij = Profile<T, PROF>::k(ex_d2<T, DP>(xi, xs + j * DP, diff));
#pragma unroll
    for (int c = 0; c < TC; ++c) tacc[c] = ExScalar<T>::fma(kij, vs[j * TC + c], tacc[c]);
}

// the (row block, j slice) this workgroup serves and the j range of the slice
struct ExRange {
    int64_t i;       // this thread's row (may be >= n1: stages, never writes)
    int64_t jbeg, jend;
    int split;
};

__device__ __forceinline__ ExRange ex_range(int64_t n2, int splits)
{
    ExRange r;
    const int64_t rb = blockIdx.x / splits;
    r.split = (int)(blockIdx.x % splits);
    r.i = rb * kExThreads + threadIdx.x;
    const int64_t chunk = (n2 + splits - 1) / splits;
    r.jbeg = std::min<int64_t>(n2, (int64_t)r.split * chunk);
    r.jend = std::min<int64_t>(n2, r.jbeg + chunk);
    return r;
}

// out (splits == 1) or slab `split` of the workspace [splits][n1][t]: sum over the slice's j of k(d2_ij) v[j][:]
template <typename T, int PROF, int DP, int TC>
__global__ __launch_bounds__(kExThreads) void exact_mvm_kernel(const T *__restrict__ x1, int64_t n1, const T *__restrict__ x2,
                                                               int64_t n2, int d, const T *__restrict__ v, int t,
                                                               T *__restrict__ out, int splits)
{
    constexpr int kTileJ = ExScalar<T>::kTileJ;
    __shared__ __align__(16) T xs[kTileJ * DP];
    __shared__ __align__(16) T vs[kTileJ * TC];
    const ExRange r = ex_range(n2, splits);
    const bool live = r.i < n1;
    T xi[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xi[k] = (live && k < d) ? x1[r.i * d + k] : T(0);
    T *dst = out + (size_t)r.split * (size_t)n1 * t;
    for (int c0 = 0; c0 < t; c0 += TC) {
        T acc[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = T(0);
        for (int64_t j0 = r.jbeg; j0 < r.jend; j0 += kTileJ) {
            const int jn = (int)std::min<int64_t>(kTileJ, r.jend - j0);
            __syncthreads();
            ex_stage<T, DP, TC>(x2, v, d, t, j0, jn, c0, xs, vs);
            __syncthreads();
            // a tile's sum apart from the running one: blocked summation (the rounding error grows with the tile and
            // the tile count, not with the whole j range)
            T tacc[TC];
#pragma unroll
            for (int c = 0; c < TC; ++c) tacc[c] = T(0);
            if constexpr (ExScalar<T>::kUnrollForward) {
#pragma unroll 2
                for (int j = 0; j < jn; ++j) ex_mvm_pair<T, PROF, DP, TC>(xi, xs, vs, j, tacc);
            } else {
                for (int j = 0; j < jn; ++j) ex_mvm_pair<T, PROF, DP, TC>(xi, xs, vs, j, tacc);
            }
#pragma unroll
            for (int c = 0; c < TC; ++c) acc[c] += tacc[c];
        }
        if (live) {
#pragma unroll
            for (int c = 0; c < TC; ++c)
                if (c0 + c < t) dst[r.i * t + c0 + c] = acc[c];
        }
    }
}

// grad (splits == 1) or slab `split` of [splits][n1][d]: sum over the slice's j of 2 k'(d2_ij) (x1_i - x2_j) (g_i . v_j)
template <typename T, int PROF, int DP, int TC>
__global__ __launch_bounds__(kExThreads) void exact_grad_kernel(const T *__restrict__ x1, int64_t n1, const T *__restrict__ x2,
                                                                int64_t n2, int d, const T *__restrict__ g,
                                                                const T *__restrict__ v, int t, T *__restrict__ grad, int splits)
{
    constexpr int kTileJ = ExScalar<T>::kTileJ;
    __shared__ __align__(16) T xs[kTileJ * DP];
    __shared__ __align__(16) T vs[kTileJ * TC];
    const ExRange r = ex_range(n2, splits);
    const bool live = r.i < n1;
    T xi[DP], acc[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
        xi[k] = (live && k < d) ? x1[r.i * d + k] : T(0);
        acc[k] = T(0);
    }
    for (int c0 = 0; c0 < t; c0 += TC) {
        T gi[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) gi[c] = (live && c0 + c < t) ? g[r.i * t + c0 + c] : T(0);
        for (int64_t j0 = r.jbeg; j0 < r.jend; j0 += kTileJ) {
            const int jn = (int)std::min<int64_t>(kTileJ, r.jend - j0);
            __syncthreads();
            ex_stage<T, DP, TC>(x2, v, d, t, j0, jn, c0, xs, vs);
            __syncthreads();
            T tacc[DP];
#pragma unroll
            for (int k = 0; k < DP; ++k) tacc[k] = T(0);
            for (int j = 0; j < jn; ++j) {
                T diff[DP];
                const T d2 = ex_d2<T, DP>(xi, xs + j * DP, diff);
                T dot = T(0);
#pragma unroll
                for (int c = 0; c < TC; ++c) dot = ExScalar<T>::fma(gi[c], vs[j * TC + c], dot);
                const T w = Profile<T, PROF>::dk2(d2) * dot;
#pragma unroll
                for (int k = 0; k < DP; ++k) tacc[k] = ExScalar<T>::fma(w, diff[k], tacc[k]);
            }
#pragma unroll
            for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
        }
    }
    if (live) {
        T *dst = grad + (size_t)r.split * (size_t)n1 * d;
#pragma unroll
        for (int k = 0; k < DP; ++k)
            if (k < d) dst[r.i * d + k] = acc[k];
    }
}

// out[e] = sum over s < splits of work[s][e], in slice order
template <typename T>
__global__ __launch_bounds__(kExThreads) void exact_sum_slabs_kernel(const T *__restrict__ work, int64_t count, int splits,
                                                                     T *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * kExThreads + threadIdx.x;
    if (e >= count) return;
    T s = work[e];
    for (int k = 1; k < splits; ++k) s += work[(size_t)k * count + e];
    out[e] = s;
}

// the rows of the partial slabs the workspace is sized for.  The workspace bound is monotone in every size (min / max of
// monotone terms), at most 16 MiB, and holds the slabs of every split ex_splits chooses.
static int64_t ex_split_rows(int64_t n1, int64_t n2)
{
    const int64_t per_row = std::min<int64_t>(kExMaxSplits, std::max<int64_t>(1, n2 / kExSplitJ));
    return std::min(n1 * per_row, std::max(n1, kExSplitRowCap));
}

template <typename T> constexpr int64_t kExWorkCap = kExWorkBytesCap / (int64_t)sizeof(T);      // the 16 MiB in elements

// the workspace in bytes, or -1 for sizes no entry point accepts
template <typename T>
static int64_t ex_work_bytes(int64_t n1, int64_t n2, int d, int t)
{
    if (n1 < 1 || n2 < 1 || n1 >= kExMaxRows || n2 >= kExMaxRows || d < 1 || d > PLX_MAX_DIM || t < 1) return -1;
    const int64_t w = std::max(d, t);
    return (int64_t)sizeof(T) * std::min(w * ex_split_rows(n1, n2), kExWorkCap<T>);
}

// splits of the j range for this call: enough workgroups to fill the chip, slabs within the workspace bound
template <typename T>
static int ex_splits(int64_t n1, int64_t n2, int d, int t)
{
    if (ex_work_bytes<T>(n1, n2, d, t) < 0) return -1;
    const int64_t w = std::max(d, t);
    const int64_t rows = std::min(ex_split_rows(n1, n2), std::min(kExSplitRowCap, kExWorkCap<T> / w));
    const int64_t blocks = ceil_div(n1, (int64_t)kExThreads);
    const int64_t want = ceil_div((int64_t)2048, blocks);
    const int64_t s = std::min(want, rows / n1);
    return (int)std::max<int64_t>(1, s);
}

static int ex_dp(int d)
{
    if (d <= 4) return 4;
    if (d <= 8) return 8;
    if (d <= 12) return 12;
    if (d <= 16) return 16;
    if (d <= 20) return 20;
    if (d <= 24) return 24;
    return 32;
}

static int ex_tc(int t)
{
    if (t <= 1) return 1;
    if (t <= 4) return 4;
    if (t <= 8) return 8;
    return 16;
}

// what a launch takes, handed down the three dispatch levels; g is unused by the forward
template <typename T> struct ExArgs {
    bool grad;
    const T *x1;
    int64_t n1;
    const T *x2;
    int64_t n2;
    int d;
    const T *g, *v;
    int t;
    T *dst;
    int splits;
    hipStream_t s;
};

template <typename T, int PROF, int DP, int TC>
static void ex_launch(const ExArgs<T> &a)
{
    const unsigned blocks = (unsigned)(ceil_div(a.n1, (int64_t)kExThreads) * a.splits);
    if (a.grad)
        exact_grad_kernel<T, PROF, DP, TC><<<blocks, kExThreads, 0, a.s>>>(a.x1, a.n1, a.x2, a.n2, a.d, a.g, a.v, a.t, a.dst, a.splits);
    else
        exact_mvm_kernel<T, PROF, DP, TC><<<blocks, kExThreads, 0, a.s>>>(a.x1, a.n1, a.x2, a.n2, a.d, a.v, a.t, a.dst, a.splits);
}

template <typename T, int PROF, int DP>
static void ex_dispatch_tc(const ExArgs<T> &a)
{
    switch (ex_tc(a.t)) {
    case 1: ex_launch<T, PROF, DP, 1>(a); break;
    case 4: ex_launch<T, PROF, DP, 4>(a); break;
    case 8: ex_launch<T, PROF, DP, 8>(a); break;
    default: ex_launch<T, PROF, DP, 16>(a); break;
    }
}

template <typename T, int PROF>
static void ex_dispatch_dp(const ExArgs<T> &a)
{
    switch (ex_dp(a.d)) {
    case 4: ex_dispatch_tc<T, PROF, 4>(a); break;
    case 8: ex_dispatch_tc<T, PROF, 8>(a); break;
    case 12: ex_dispatch_tc<T, PROF, 12>(a); break;
    case 16: ex_dispatch_tc<T, PROF, 16>(a); break;
    case 20: ex_dispatch_tc<T, PROF, 20>(a); break;
    case 24: ex_dispatch_tc<T, PROF, 24>(a); break;
    default: ex_dispatch_tc<T, PROF, 32>(a); break;
    }
}

// the checks every entry point makes before any GPU work
template <typename T>
static int ex_check(const char *who, const T *x1, int64_t n1, const T *x2, int64_t n2, int d, int profile, const T *a, const T *b,
                    int t, const T *dst, const void *work, int64_t work_bytes)
{
    if (!x1 || !x2 || !a || !b || !dst || !work) {
        set_error("%s: NULL argument", who);
        return PLX_ERR_INVALID;
    }
    if (n1 < 1 || n2 < 1 || n1 >= kExMaxRows || n2 >= kExMaxRows) {
        set_error("%s: n1 = %lld, n2 = %lld outside 1..2^31-1", who, (long long)n1, (long long)n2);
        return PLX_ERR_INVALID;
    }
    if (d < 1 || d > PLX_MAX_DIM) {
        set_error("%s: d = %d outside 1..%d", who, d, PLX_MAX_DIM);
        return PLX_ERR_DIM;
    }
    if (profile < PLX_PROFILE_RBF || profile > PLX_PROFILE_MATERN52) {
        set_error("%s: unknown profile %d", who, profile);
        return PLX_ERR_INVALID;
    }
    if (t < 1) {
        set_error("%s: t = %d columns, at least 1", who, t);
        return PLX_ERR_INVALID;
    }
    const int64_t need = ex_work_bytes<T>(n1, n2, d, t);
    if (work_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (%s)", who, (long long)work_bytes, (long long)need,
                  ExScalar<T>::kWorkBytes);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

// either entry point: the checks, the templated kernel into dst or the slabs, the slab sum (g is NULL in the forward)
template <typename T>
static int ex_run(const char *who, bool grad, const T *x1, int64_t n1, const T *x2, int64_t n2, int d, int profile, const T *g,
                  const T *v, int t, T *dst, void *work, int64_t work_bytes, void *stream)
{
    PLX_TRY(ex_check<T>(who, x1, n1, x2, n2, d, profile, grad ? g : v, v, t, dst, work, work_bytes));
    const int splits = ex_splits<T>(n1, n2, d, t);          // the query the header documents: it cannot drift from the launch
    T *target = splits > 1 ? reinterpret_cast<T *>(work) : dst;
    const ExArgs<T> a{grad, x1, n1, x2, n2, d, g, v, t, target, splits, (hipStream_t)stream};
    switch (profile) {
    case PLX_PROFILE_RBF: ex_dispatch_dp<T, PLX_PROFILE_RBF>(a); break;
    case PLX_PROFILE_MATERN12: ex_dispatch_dp<T, PLX_PROFILE_MATERN12>(a); break;
    case PLX_PROFILE_MATERN32: ex_dispatch_dp<T, PLX_PROFILE_MATERN32>(a); break;
    default: ex_dispatch_dp<T, PLX_PROFILE_MATERN52>(a); break;
    }
    PLX_HIP_TRY(hipGetLastError());
    if (splits > 1) {
        const int64_t count = n1 * (grad ? d : t);
        exact_sum_slabs_kernel<T><<<(unsigned)ceil_div(count, (int64_t)kExThreads), kExThreads, 0, a.s>>>(target, count, splits, dst);
        PLX_HIP_TRY(hipGetLastError());
    }
    return PLX_OK;
}

}  // namespace plx
