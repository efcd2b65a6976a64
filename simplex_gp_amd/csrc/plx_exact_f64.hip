// plx_exact_f64.hip -- the exact kernel MVM and its position gradient with every array and every operation in double:
//
//   out[i][c]     = sum_j k(|x1_i - x2_j|^2) v[j][c]                                        plx_exact_mvm_f64
//   grad_x1[i][:] = sum_j 2 k'(|x1_i - x2_j|^2) (x1_i - x2_j) (g_i . v_j)                   plx_exact_grad_f64
//
// The formulas, the profiles and the conventions are those of plx_exact.hip (2 k' of Matern-1/2 is 0 at r = 0, direct
// differences, each tile summed apart from the running sum); so is the contract (stateless, the caller's workspace, no
// float atomics, every output element written by one thread, graph-capturable).  Nothing passes through fp32: exp and
// sqrt are the double library functions, the Matern constants double literals.
//
// Layout.  A workgroup of 256 threads owns 256 consecutive rows i, one per thread; x1_i (zero-padded to DP, a multiple
// of 4 >= d) and the row's accumulators stay in registers (two 32-bit registers per value).  The j range is walked in
// tiles of kEx64TileJ = 64 rows of x2 and of a column block of v (TC columns) staged in LDS: 64 rows of doubles are the
// bytes of the fp32 kernel's 128 rows (at most 16 + 8 KiB), and the tile's sequential sum -- the largest term of the
// rounding bound of an entry -- is half as long.  Every thread reads the same LDS words (broadcast ds_read_b128, two
// doubles each).  The DP and TC ladders are the fp32 kernel's: a padded dimension costs a subtraction and an FMA at the
// double rate, so the fine DP ladder matters more here, and TC = 16 keeps t = 11 in one column block (the forward
// recomputes k, a software exp, per block).
//
// Cost model (VALU, per pair and lane, in double-rate instructions): DP subtractions + DP FMAs for d2, the software exp
// (gfx950 has no double exponential: argument reduction, a degree-11 polynomial and the scaling, counted in DESIGN.md
// section 20), a Newton square root for the Materns, TC FMAs for the contraction.
//
// Split j as in plx_exact.hip: slabs [splits][n1][t or d] of doubles in the caller's workspace, summed in slice order by
// a second kernel.  The workspace bound is in bytes and at most 16 MiB, so the cap allows half the fp32 kernel's elements.
#include "plx_internal.h"

#include <algorithm>

namespace plx {

constexpr int kEx64Threads = 256;                 // rows per workgroup, one per thread
constexpr int kEx64TileJ = 64;                    // x2 / v rows per LDS tile
constexpr int64_t kEx64MaxRows = (int64_t)1 << 31;            // n1, n2 < 2^31
constexpr int64_t kEx64SplitRowCap = 524288;      // split only while splits * n1 <= this many rows ...
constexpr int64_t kEx64WorkDoublesCap = (int64_t)1 << 21;     // ... and the slabs fit 16 MiB
constexpr int kEx64MaxSplits = 1024;
constexpr int kEx64SplitJ = 512;                  // a slice covers at least this many j

template <int P> struct Profile64;

// RBF: k = exp(-d2); 2 k' = -2 exp(-d2)
template <> struct Profile64<PLX_PROFILE_RBF> {
    static __device__ __forceinline__ double k(double d2) { return exp(-d2); }
    static __device__ __forceinline__ double dk2(double d2) { return -2.0 * exp(-d2); }
};
// Matern-1/2: k = e^-r; 2 k' = -e^-r / r, singular at r = 0, where the pair contributes 0 (x1_i - x2_j = 0 there)
template <> struct Profile64<PLX_PROFILE_MATERN12> {
    static __device__ __forceinline__ double k(double d2) { return exp(-sqrt(d2)); }
    static __device__ __forceinline__ double dk2(double d2)
    {
        const double r = sqrt(d2);
        return r > 0.0 ? -exp(-r) / r : 0.0;
    }
};
// Matern-3/2: k = (1 + sqrt3 r) e^{-sqrt3 r}; 2 k' = -3 e^{-sqrt3 r}
template <> struct Profile64<PLX_PROFILE_MATERN32> {
    static __device__ __forceinline__ double k(double d2)
    {
        const double s = 1.7320508075688772 * sqrt(d2);
        return (1.0 + s) * exp(-s);
    }
    static __device__ __forceinline__ double dk2(double d2) { return -3.0 * exp(-1.7320508075688772 * sqrt(d2)); }
};
// Matern-5/2: k = (1 + sqrt5 r + 5/3 r^2) e^{-sqrt5 r}; 2 k' = -(5/3) (1 + sqrt5 r) e^{-sqrt5 r}
template <> struct Profile64<PLX_PROFILE_MATERN52> {
    static __device__ __forceinline__ double k(double d2)
    {
        const double s = 2.2360679774997896 * sqrt(d2);
        return (1.0 + s + (5.0 / 3.0) * d2) * exp(-s);
    }
    static __device__ __forceinline__ double dk2(double d2)
    {
        const double s = 2.2360679774997896 * sqrt(d2);
        return (-5.0 / 3.0) * (1.0 + s) * exp(-s);
    }
};

// the workgroup's tile of x2 rows [j0, j0 + jn) into LDS, zero-padded to DP columns; and of column block [c0, c0 + TC)
// of v (zero past t).  Rows past jn are never read.
template <int DP, int TC>
__device__ __forceinline__ void ex64_stage(const double *__restrict__ x2, const double *__restrict__ v, int d, int t, int64_t j0,
                                           int jn, int c0, double *xs, double *vs)
{
    for (int e = threadIdx.x; e < kEx64TileJ * DP; e += kEx64Threads) {
        const int j = e / DP, k = e % DP;
        xs[e] = (j < jn && k < d) ? x2[(j0 + j) * d + k] : 0.0;
    }
    for (int e = threadIdx.x; e < kEx64TileJ * TC; e += kEx64Threads) {
        const int j = e / TC, c = e % TC;
        vs[e] = (j < jn && c0 + c < t) ? v[(j0 + j) * t + c0 + c] : 0.0;
    }
}

template <int DP>
__device__ __forceinline__ double ex64_d2(const double (&xi)[DP], const double *xj)
{
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < DP; k += 2) {
        const double2 b = *reinterpret_cast<const double2 *>(xj + k);
        const double e0 = xi[k] - b.x, e1 = xi[k + 1] - b.y;
        d2 = fma(e0, e0, d2);
        d2 = fma(e1, e1, d2);
    }
    return d2;
}

// the (row block, j slice) this workgroup serves and the j range of the slice
struct Ex64Range {
    int64_t i;       // this thread's row (may be >= n1: stages, never writes)
    int64_t jbeg, jend;
    int split;
};

__device__ __forceinline__ Ex64Range ex64_range(int64_t n2, int splits)
{
    Ex64Range r;
    const int64_t rb = blockIdx.x / splits;
    r.split = (int)(blockIdx.x % splits);
    r.i = rb * kEx64Threads + threadIdx.x;
    const int64_t chunk = (n2 + splits - 1) / splits;
    r.jbeg = std::min<int64_t>(n2, (int64_t)r.split * chunk);
    r.jend = std::min<int64_t>(n2, r.jbeg + chunk);
    return r;
}

// out (splits == 1) or slab `split` of the workspace [splits][n1][t]: sum over the slice's j of k(d2_ij) v[j][:]
template <int PROF, int DP, int TC>
__global__ __launch_bounds__(kEx64Threads) void exact64_mvm_kernel(const double *__restrict__ x1, int64_t n1,
                                                                   const double *__restrict__ x2, int64_t n2, int d,
                                                                   const double *__restrict__ v, int t,
                                                                   double *__restrict__ out, int splits)
{
    __shared__ __align__(16) double xs[kEx64TileJ * DP];
    __shared__ __align__(16) double vs[kEx64TileJ * TC];
    const Ex64Range r = ex64_range(n2, splits);
    const bool live = r.i < n1;
    double xi[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xi[k] = (live && k < d) ? x1[r.i * d + k] : 0.0;
    double *dst = out + (size_t)r.split * (size_t)n1 * t;
    for (int c0 = 0; c0 < t; c0 += TC) {
        double acc[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = 0.0;
        for (int64_t j0 = r.jbeg; j0 < r.jend; j0 += kEx64TileJ) {
            const int jn = (int)std::min<int64_t>(kEx64TileJ, r.jend - j0);
            __syncthreads();
            ex64_stage<DP, TC>(x2, v, d, t, j0, jn, c0, xs, vs);
            __syncthreads();
            // a tile's sum apart from the running one: blocked summation (the rounding error grows with the tile and
            // the tile count, not with the whole j range)
            double tacc[TC];
#pragma unroll
            for (int c = 0; c < TC; ++c) tacc[c] = 0.0;
            for (int j = 0; j < jn; ++j) {
                const double kij = Profile64<PROF>::k(ex64_d2<DP>(xi, xs + j * DP));
#pragma unroll
                for (int c = 0; c < TC; ++c) tacc[c] = fma(kij, vs[j * TC + c], tacc[c]);
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
template <int PROF, int DP, int TC>
__global__ __launch_bounds__(kEx64Threads) void exact64_grad_kernel(const double *__restrict__ x1, int64_t n1,
                                                                    const double *__restrict__ x2, int64_t n2, int d,
                                                                    const double *__restrict__ g, const double *__restrict__ v,
                                                                    int t, double *__restrict__ grad, int splits)
{
    __shared__ __align__(16) double xs[kEx64TileJ * DP];
    __shared__ __align__(16) double vs[kEx64TileJ * TC];
    const Ex64Range r = ex64_range(n2, splits);
    const bool live = r.i < n1;
    double xi[DP], acc[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
        xi[k] = (live && k < d) ? x1[r.i * d + k] : 0.0;
        acc[k] = 0.0;
    }
    for (int c0 = 0; c0 < t; c0 += TC) {
        double gi[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) gi[c] = (live && c0 + c < t) ? g[r.i * t + c0 + c] : 0.0;
        for (int64_t j0 = r.jbeg; j0 < r.jend; j0 += kEx64TileJ) {
            const int jn = (int)std::min<int64_t>(kEx64TileJ, r.jend - j0);
            __syncthreads();
            ex64_stage<DP, TC>(x2, v, d, t, j0, jn, c0, xs, vs);
            __syncthreads();
            double tacc[DP];
#pragma unroll
            for (int k = 0; k < DP; ++k) tacc[k] = 0.0;
            for (int j = 0; j < jn; ++j) {
                const double *xj = xs + j * DP;
                double diff[DP];
                double d2 = 0.0;
#pragma unroll
                for (int k = 0; k < DP; k += 2) {
                    const double2 b = *reinterpret_cast<const double2 *>(xj + k);
                    diff[k] = xi[k] - b.x;
                    diff[k + 1] = xi[k + 1] - b.y;
                    d2 = fma(diff[k], diff[k], d2);
                    d2 = fma(diff[k + 1], diff[k + 1], d2);
                }
                double dot = 0.0;
#pragma unroll
                for (int c = 0; c < TC; ++c) dot = fma(gi[c], vs[j * TC + c], dot);
                const double w = Profile64<PROF>::dk2(d2) * dot;
#pragma unroll
                for (int k = 0; k < DP; ++k) tacc[k] = fma(w, diff[k], tacc[k]);
            }
#pragma unroll
            for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
        }
    }
    if (live) {
        double *dst = grad + (size_t)r.split * (size_t)n1 * d;
#pragma unroll
        for (int k = 0; k < DP; ++k)
            if (k < d) dst[r.i * d + k] = acc[k];
    }
}

// out[e] = sum over s < splits of work[s][e], in slice order
__global__ __launch_bounds__(kEx64Threads) void exact64_sum_slabs_kernel(const double *__restrict__ work, int64_t count,
                                                                         int splits, double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * kEx64Threads + threadIdx.x;
    if (e >= count) return;
    double s = work[e];
    for (int k = 1; k < splits; ++k) s += work[(size_t)k * count + e];
    out[e] = s;
}

// the rows of the partial slabs the workspace is sized for.  The workspace bound is monotone in every size (min / max of
// monotone terms), at most 16 MiB, and holds the slabs of every split ex64_splits chooses.
static int64_t ex64_split_rows(int64_t n1, int64_t n2)
{
    const int64_t per_row = std::min<int64_t>(kEx64MaxSplits, std::max<int64_t>(1, n2 / kEx64SplitJ));
    return std::min(n1 * per_row, std::max(n1, kEx64SplitRowCap));
}

static int64_t ex64_work_doubles(int64_t n1, int64_t n2, int d, int t)
{
    const int64_t w = std::max(d, t);
    return std::min(w * ex64_split_rows(n1, n2), kEx64WorkDoublesCap);
}

// splits of the j range for this call: enough workgroups to fill the chip, slabs within the workspace bound
static int ex64_splits(int64_t n1, int64_t n2, int d, int t)
{
    const int64_t w = std::max(d, t);
    const int64_t rows = std::min(ex64_split_rows(n1, n2), std::min(kEx64SplitRowCap, kEx64WorkDoublesCap / w));
    const int64_t blocks = ceil_div(n1, (int64_t)kEx64Threads);
    const int64_t want = ceil_div((int64_t)2048, blocks);
    const int64_t s = std::min(want, rows / n1);
    return (int)std::max<int64_t>(1, s);
}

static int ex64_dp(int d)
{
    if (d <= 4) return 4;
    if (d <= 8) return 8;
    if (d <= 12) return 12;
    if (d <= 16) return 16;
    if (d <= 20) return 20;
    if (d <= 24) return 24;
    return 32;
}

static int ex64_tc(int t)
{
    if (t <= 1) return 1;
    if (t <= 4) return 4;
    if (t <= 8) return 8;
    return 16;
}

template <int PROF, int DP, int TC>
static void ex64_launch(bool grad, const double *x1, int64_t n1, const double *x2, int64_t n2, int d, const double *g,
                        const double *v, int t, double *dst, int splits, hipStream_t s)
{
    const unsigned blocks = (unsigned)(ceil_div(n1, (int64_t)kEx64Threads) * splits);
    if (grad)
        exact64_grad_kernel<PROF, DP, TC><<<blocks, kEx64Threads, 0, s>>>(x1, n1, x2, n2, d, g, v, t, dst, splits);
    else
        exact64_mvm_kernel<PROF, DP, TC><<<blocks, kEx64Threads, 0, s>>>(x1, n1, x2, n2, d, v, t, dst, splits);
}

template <int PROF, int DP>
static void ex64_dispatch_tc(bool grad, const double *x1, int64_t n1, const double *x2, int64_t n2, int d, const double *g,
                             const double *v, int t, double *dst, int splits, hipStream_t s)
{
    switch (ex64_tc(t)) {
    case 1: ex64_launch<PROF, DP, 1>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 4: ex64_launch<PROF, DP, 4>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 8: ex64_launch<PROF, DP, 8>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    default: ex64_launch<PROF, DP, 16>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    }
}

template <int PROF>
static void ex64_dispatch_dp(bool grad, const double *x1, int64_t n1, const double *x2, int64_t n2, int d, const double *g,
                             const double *v, int t, double *dst, int splits, hipStream_t s)
{
    switch (ex64_dp(d)) {
    case 4: ex64_dispatch_tc<PROF, 4>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 8: ex64_dispatch_tc<PROF, 8>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 12: ex64_dispatch_tc<PROF, 12>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 16: ex64_dispatch_tc<PROF, 16>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 20: ex64_dispatch_tc<PROF, 20>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 24: ex64_dispatch_tc<PROF, 24>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    default: ex64_dispatch_tc<PROF, 32>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    }
}

// the checks every entry point makes before any GPU work: those of plx_exact.hip's ex_check, in its order
static int ex64_check(const char *who, const double *x1, int64_t n1, const double *x2, int64_t n2, int d, int profile,
                      const double *a, const double *b, int t, const double *dst, const void *work, int64_t work_bytes)
{
    if (!x1 || !x2 || !a || !b || !dst || !work) {
        set_error("%s: NULL argument", who);
        return PLX_ERR_INVALID;
    }
    if (n1 < 1 || n2 < 1 || n1 >= kEx64MaxRows || n2 >= kEx64MaxRows) {
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
    const int64_t need = plx_exact_work_bytes_f64(n1, n2, d, t);
    if (work_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (plx_exact_work_bytes_f64)", who, (long long)work_bytes,
                  (long long)need);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

static int ex64_run(bool grad, const double *x1, int64_t n1, const double *x2, int64_t n2, int d, int profile, const double *g,
                    const double *v, int t, double *dst, void *work, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int splits = plx_exact_splits_f64(n1, n2, d, t);  // the query the header documents: it cannot drift from the launch
    double *target = splits > 1 ? reinterpret_cast<double *>(work) : dst;
    switch (profile) {
    case PLX_PROFILE_RBF: ex64_dispatch_dp<PLX_PROFILE_RBF>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    case PLX_PROFILE_MATERN12: ex64_dispatch_dp<PLX_PROFILE_MATERN12>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    case PLX_PROFILE_MATERN32: ex64_dispatch_dp<PLX_PROFILE_MATERN32>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    default: ex64_dispatch_dp<PLX_PROFILE_MATERN52>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    }
    PLX_HIP_TRY(hipGetLastError());
    if (splits > 1) {
        const int64_t count = n1 * (grad ? d : t);
        exact64_sum_slabs_kernel<<<(unsigned)ceil_div(count, (int64_t)kEx64Threads), kEx64Threads, 0, s>>>(target, count, splits,
                                                                                                        dst);
        PLX_HIP_TRY(hipGetLastError());
    }
    return PLX_OK;
}

}  // namespace plx

using namespace plx;

extern "C" int64_t plx_exact_work_bytes_f64(int64_t n1, int64_t n2, int d, int t)
{
    if (n1 < 1 || n2 < 1 || n1 >= kEx64MaxRows || n2 >= kEx64MaxRows || d < 1 || d > PLX_MAX_DIM || t < 1) return -1;
    return 8 * ex64_work_doubles(n1, n2, d, t);
}

extern "C" int plx_exact_splits_f64(int64_t n1, int64_t n2, int d, int t)
{
    if (plx_exact_work_bytes_f64(n1, n2, d, t) < 0) return -1;
    return ex64_splits(n1, n2, d, t);
}

extern "C" int plx_exact_mvm_f64(const double *d_x1, int64_t n1, const double *d_x2, int64_t n2, int d, int profile,
                                 const double *d_v, int t, double *d_out, void *d_work, int64_t work_bytes, void *stream)
{
    PLX_TRY(ex64_check("plx_exact_mvm_f64", d_x1, n1, d_x2, n2, d, profile, d_v, d_v, t, d_out, d_work, work_bytes));
    return ex64_run(false, d_x1, n1, d_x2, n2, d, profile, nullptr, d_v, t, d_out, d_work, stream);
}

extern "C" int plx_exact_grad_f64(const double *d_x1, int64_t n1, const double *d_x2, int64_t n2, int d, int profile,
                                  const double *d_g, const double *d_v, int t, double *d_grad_x1, void *d_work,
                                  int64_t work_bytes, void *stream)
{
    PLX_TRY(ex64_check("plx_exact_grad_f64", d_x1, n1, d_x2, n2, d, profile, d_g, d_v, t, d_grad_x1, d_work, work_bytes));
    return ex64_run(true, d_x1, n1, d_x2, n2, d, profile, d_g, d_v, t, d_grad_x1, d_work, stream);
}
