// plx_exact.hip -- the exact kernel MVM, evaluated on the fly (no N x N matrix is ever stored):
//
//   out[i][c]     = sum_j k(|x1_i - x2_j|^2) v[j][c]                                        plx_exact_mvm
//   grad_x1[i][:] = sum_j 2 k'(|x1_i - x2_j|^2) (x1_i - x2_j) (g_i . v_j)                   plx_exact_grad
//
// k is one of the project's profiles of the squared distance (stencil.py: rbf, matern), compiled in.  This is what the
// lattice stands in for: the yardstick of its approximation error, and the like-for-like speed figure beside it.
//
// Layout.  A workgroup of 256 threads owns 256 consecutive rows i, one per thread; x1_i (zero-padded to DP, a multiple
// of 4 >= d) and the row's accumulators stay in registers.  The j range is walked in tiles of kExTileJ rows of x2 (and of
// v, a column block of TC at a time) staged in LDS; every thread reads the same LDS words (broadcast, no bank
// conflicts).  Distances are direct differences, sum_k (x1_ik - x2_jk)^2: no norm expansion, so no cancellation for
// close points far from the origin, and d2 >= 0 by construction.
//
// Cost model (VALU, per pair and lane): DP subtractions + DP FMAs for d2, one v_exp_f32 (8 issue cycles against 4 for an
// FMA; Matern adds a v_sqrt_f32), TC FMAs for the contraction.  The operands come from LDS as broadcast dwordx4 reads.
//
// Columns: t > TC loops over column blocks; the forward recomputes k per block (its outputs are per block), the gradient
// accumulates over blocks in registers (the gradient is linear in the columns of g and v).
//
// Split j.  When n1 is small (prediction rows, n1 = 8 ...) one workgroup per 256 rows leaves the chip idle, so the j
// range is cut into `splits` slices, each written to its own slab of the caller's workspace, and a second kernel sums the
// slabs in slice order.  No float atomics: two identical calls are bitwise equal (plx.h's contract).
#include "plx_internal.h"

#include <algorithm>

namespace plx {

constexpr int kExThreads = 256;                 // rows per workgroup, one per thread
constexpr int kExTileJ = 128;                   // x2 / v rows per LDS tile
constexpr int64_t kExMaxRows = (int64_t)1 << 31;             // n1, n2 < 2^31
constexpr int64_t kExSplitRowCap = 524288;      // split only while splits * n1 <= this many rows ...
constexpr int64_t kExWorkFloatsCap = (int64_t)1 << 22;       // ... and the slabs fit 16 MB
constexpr int kExMaxSplits = 1024;
constexpr int kExSplitJ = 512;                  // a slice covers at least this many j

template <int P> struct Profile;

// RBF: k = exp(-d2) (stencil.rbf, the lattice's own RBF -- not GPyTorch's exp(-d2 / 2)); 2 k' = -2 exp(-d2)
template <> struct Profile<PLX_PROFILE_RBF> {
    static __device__ __forceinline__ float k(float d2) { return __expf(-d2); }
    static __device__ __forceinline__ float dk2(float d2) { return -2.f * __expf(-d2); }
};
// Matern-1/2: k = e^-r; 2 k' = -e^-r / r, singular at r = 0, where the pair contributes 0 (x1_i - x2_j = 0 there)
template <> struct Profile<PLX_PROFILE_MATERN12> {
    static __device__ __forceinline__ float k(float d2) { return __expf(-sqrtf(d2)); }
    static __device__ __forceinline__ float dk2(float d2)
    {
        const float r = sqrtf(d2);
        return r > 0.f ? -__expf(-r) / r : 0.f;
    }
};
// Matern-3/2: k = (1 + sqrt3 r) e^{-sqrt3 r}; 2 k' = -3 e^{-sqrt3 r}
template <> struct Profile<PLX_PROFILE_MATERN32> {
    static __device__ __forceinline__ float k(float d2)
    {
        const float s = 1.7320508075688772f * sqrtf(d2);
        return (1.f + s) * __expf(-s);
    }
    static __device__ __forceinline__ float dk2(float d2) { return -3.f * __expf(-1.7320508075688772f * sqrtf(d2)); }
};
// Matern-5/2: k = (1 + sqrt5 r + 5/3 r^2) e^{-sqrt5 r}; 2 k' = -(5/3) (1 + sqrt5 r) e^{-sqrt5 r}
template <> struct Profile<PLX_PROFILE_MATERN52> {
    static __device__ __forceinline__ float k(float d2)
    {
        const float s = 2.2360679774997896f * sqrtf(d2);
        return (1.f + s + (5.f / 3.f) * d2) * __expf(-s);
    }
    static __device__ __forceinline__ float dk2(float d2)
    {
        const float s = 2.2360679774997896f * sqrtf(d2);
        return (-5.f / 3.f) * (1.f + s) * __expf(-s);
    }
};

// the workgroup's tile of x2 rows [j0, j0 + jn) into LDS, zero-padded to DP columns; and of column block [c0, c0 + TC)
// of v (zero past t).  Rows past jn are never read.
template <int DP, int TC>
__device__ __forceinline__ void ex_stage(const float *__restrict__ x2, const float *__restrict__ v, int d, int t, int64_t j0,
                                         int jn, int c0, float *xs, float *vs)
{
    for (int e = threadIdx.x; e < kExTileJ * DP; e += kExThreads) {
        const int j = e / DP, k = e % DP;
        xs[e] = (j < jn && k < d) ? x2[(j0 + j) * d + k] : 0.f;
    }
    for (int e = threadIdx.x; e < kExTileJ * TC; e += kExThreads) {
        const int j = e / TC, c = e % TC;
        vs[e] = (j < jn && c0 + c < t) ? v[(j0 + j) * t + c0 + c] : 0.f;
    }
}

template <int DP>
__device__ __forceinline__ float ex_d2(const float (&xi)[DP], const float *xj)
{
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < DP; k += 4) {
        const float4 b = *reinterpret_cast<const float4 *>(xj + k);
        const float e0 = xi[k] - b.x, e1 = xi[k + 1] - b.y, e2 = xi[k + 2] - b.z, e3 = xi[k + 3] - b.w;
        d2 = fmaf(e0, e0, d2);
        d2 = fmaf(e1, e1, d2);
        d2 = fmaf(e2, e2, d2);
        d2 = fmaf(e3, e3, d2);
    }
    return d2;
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
template <int PROF, int DP, int TC>
__global__ __launch_bounds__(kExThreads) void exact_mvm_kernel(const float *__restrict__ x1, int64_t n1,
                                                               const float *__restrict__ x2, int64_t n2, int d,
                                                               const float *__restrict__ v, int t, float *__restrict__ out,
                                                               int splits)
{
    __shared__ __align__(16) float xs[kExTileJ * DP];
    __shared__ __align__(16) float vs[kExTileJ * TC];
    const ExRange r = ex_range(n2, splits);
    const bool live = r.i < n1;
    float xi[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xi[k] = (live && k < d) ? x1[r.i * d + k] : 0.f;
    float *dst = out + (size_t)r.split * (size_t)n1 * t;
    for (int c0 = 0; c0 < t; c0 += TC) {
        float acc[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = 0.f;
        for (int64_t j0 = r.jbeg; j0 < r.jend; j0 += kExTileJ) {
            const int jn = (int)std::min<int64_t>(kExTileJ, r.jend - j0);
            __syncthreads();
            ex_stage<DP, TC>(x2, v, d, t, j0, jn, c0, xs, vs);
            __syncthreads();
            // a tile's sum apart from the running one: blocked summation (the rounding error grows with the tile and
            // the tile count, not with the whole j range)
            float tacc[TC];
#pragma unroll
            for (int c = 0; c < TC; ++c) tacc[c] = 0.f;
#pragma unroll 2
            for (int j = 0; j < jn; ++j) {
                const float kij = Profile<PROF>::k(ex_d2<DP>(xi, xs + j * DP));
#pragma unroll
                for (int c = 0; c < TC; ++c) tacc[c] = fmaf(kij, vs[j * TC + c], tacc[c]);
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
__global__ __launch_bounds__(kExThreads) void exact_grad_kernel(const float *__restrict__ x1, int64_t n1,
                                                                const float *__restrict__ x2, int64_t n2, int d,
                                                                const float *__restrict__ g, const float *__restrict__ v,
                                                                int t, float *__restrict__ grad, int splits)
{
    __shared__ __align__(16) float xs[kExTileJ * DP];
    __shared__ __align__(16) float vs[kExTileJ * TC];
    const ExRange r = ex_range(n2, splits);
    const bool live = r.i < n1;
    float xi[DP], acc[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
        xi[k] = (live && k < d) ? x1[r.i * d + k] : 0.f;
        acc[k] = 0.f;
    }
    for (int c0 = 0; c0 < t; c0 += TC) {
        float gi[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) gi[c] = (live && c0 + c < t) ? g[r.i * t + c0 + c] : 0.f;
        for (int64_t j0 = r.jbeg; j0 < r.jend; j0 += kExTileJ) {
            const int jn = (int)std::min<int64_t>(kExTileJ, r.jend - j0);
            __syncthreads();
            ex_stage<DP, TC>(x2, v, d, t, j0, jn, c0, xs, vs);
            __syncthreads();
            float tacc[DP];
#pragma unroll
            for (int k = 0; k < DP; ++k) tacc[k] = 0.f;
            for (int j = 0; j < jn; ++j) {
                const float *xj = xs + j * DP;
                float diff[DP];
                float d2 = 0.f;
#pragma unroll
                for (int k = 0; k < DP; k += 4) {
                    const float4 b = *reinterpret_cast<const float4 *>(xj + k);
                    diff[k] = xi[k] - b.x;
                    diff[k + 1] = xi[k + 1] - b.y;
                    diff[k + 2] = xi[k + 2] - b.z;
                    diff[k + 3] = xi[k + 3] - b.w;
                    d2 = fmaf(diff[k], diff[k], d2);
                    d2 = fmaf(diff[k + 1], diff[k + 1], d2);
                    d2 = fmaf(diff[k + 2], diff[k + 2], d2);
                    d2 = fmaf(diff[k + 3], diff[k + 3], d2);
                }
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < TC; ++c) dot = fmaf(gi[c], vs[j * TC + c], dot);
                const float w = Profile<PROF>::dk2(d2) * dot;
#pragma unroll
                for (int k = 0; k < DP; ++k) tacc[k] = fmaf(w, diff[k], tacc[k]);
            }
#pragma unroll
            for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
        }
    }
    if (live) {
        float *dst = grad + (size_t)r.split * (size_t)n1 * d;
#pragma unroll
        for (int k = 0; k < DP; ++k)
            if (k < d) dst[r.i * d + k] = acc[k];
    }
}

// out[e] = sum over s < splits of work[s][e], in slice order
__global__ __launch_bounds__(kExThreads) void exact_sum_slabs_kernel(const float *__restrict__ work, int64_t count, int splits,
                                                                     float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * kExThreads + threadIdx.x;
    if (e >= count) return;
    float s = work[e];
    for (int k = 1; k < splits; ++k) s += work[(size_t)k * count + e];
    out[e] = s;
}

// the rows of the partial slabs the workspace is sized for.  The workspace bound is monotone in every size (min / max of
// monotone terms), at most 16 MB, and holds the slabs of every split ex_splits chooses.
static int64_t ex_split_rows(int64_t n1, int64_t n2)
{
    const int64_t per_row = std::min<int64_t>(kExMaxSplits, std::max<int64_t>(1, n2 / kExSplitJ));
    return std::min(n1 * per_row, std::max(n1, kExSplitRowCap));
}

static int64_t ex_work_floats(int64_t n1, int64_t n2, int d, int t)
{
    const int64_t w = std::max(d, t);
    return std::min(w * ex_split_rows(n1, n2), kExWorkFloatsCap);
}

// splits of the j range for this call: enough workgroups to fill the chip, slabs within the workspace bound
static int ex_splits(int64_t n1, int64_t n2, int d, int t)
{
    const int64_t w = std::max(d, t);
    const int64_t rows = std::min(ex_split_rows(n1, n2), std::min(kExSplitRowCap, kExWorkFloatsCap / w));
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

template <int PROF, int DP, int TC>
static void ex_launch(bool grad, const float *x1, int64_t n1, const float *x2, int64_t n2, int d, const float *g, const float *v,
                      int t, float *dst, int splits, hipStream_t s)
{
    const unsigned blocks = (unsigned)(ceil_div(n1, (int64_t)kExThreads) * splits);
    if (grad)
        exact_grad_kernel<PROF, DP, TC><<<blocks, kExThreads, 0, s>>>(x1, n1, x2, n2, d, g, v, t, dst, splits);
    else
        exact_mvm_kernel<PROF, DP, TC><<<blocks, kExThreads, 0, s>>>(x1, n1, x2, n2, d, v, t, dst, splits);
}

template <int PROF, int DP>
static void ex_dispatch_tc(bool grad, const float *x1, int64_t n1, const float *x2, int64_t n2, int d, const float *g,
                           const float *v, int t, float *dst, int splits, hipStream_t s)
{
    switch (ex_tc(t)) {
    case 1: ex_launch<PROF, DP, 1>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 4: ex_launch<PROF, DP, 4>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 8: ex_launch<PROF, DP, 8>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    default: ex_launch<PROF, DP, 16>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    }
}

template <int PROF>
static void ex_dispatch_dp(bool grad, const float *x1, int64_t n1, const float *x2, int64_t n2, int d, const float *g,
                           const float *v, int t, float *dst, int splits, hipStream_t s)
{
    switch (ex_dp(d)) {
    case 4: ex_dispatch_tc<PROF, 4>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 8: ex_dispatch_tc<PROF, 8>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 12: ex_dispatch_tc<PROF, 12>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 16: ex_dispatch_tc<PROF, 16>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 20: ex_dispatch_tc<PROF, 20>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    case 24: ex_dispatch_tc<PROF, 24>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    default: ex_dispatch_tc<PROF, 32>(grad, x1, n1, x2, n2, d, g, v, t, dst, splits, s); break;
    }
}

// the checks every entry point makes before any GPU work
static int ex_check(const char *who, const float *x1, int64_t n1, const float *x2, int64_t n2, int d, int profile, const float *a,
                    const float *b, int t, const float *dst, const void *work, int64_t work_bytes)
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
    const int64_t need = plx_exact_work_bytes(n1, n2, d, t);
    if (work_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (plx_exact_work_bytes)", who, (long long)work_bytes, (long long)need);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

static int ex_run(bool grad, const float *x1, int64_t n1, const float *x2, int64_t n2, int d, int profile, const float *g,
                  const float *v, int t, float *dst, void *work, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int splits = plx_exact_splits(n1, n2, d, t);      // the query the header documents: it cannot drift from the launch
    float *target = splits > 1 ? reinterpret_cast<float *>(work) : dst;
    switch (profile) {
    case PLX_PROFILE_RBF: ex_dispatch_dp<PLX_PROFILE_RBF>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    case PLX_PROFILE_MATERN12: ex_dispatch_dp<PLX_PROFILE_MATERN12>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    case PLX_PROFILE_MATERN32: ex_dispatch_dp<PLX_PROFILE_MATERN32>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    default: ex_dispatch_dp<PLX_PROFILE_MATERN52>(grad, x1, n1, x2, n2, d, g, v, t, target, splits, s); break;
    }
    PLX_HIP_TRY(hipGetLastError());
    if (splits > 1) {
        const int64_t count = n1 * (grad ? d : t);
        exact_sum_slabs_kernel<<<(unsigned)ceil_div(count, (int64_t)kExThreads), kExThreads, 0, s>>>(target, count, splits, dst);
        PLX_HIP_TRY(hipGetLastError());
    }
    return PLX_OK;
}

}  // namespace plx

using namespace plx;

extern "C" int64_t plx_exact_work_bytes(int64_t n1, int64_t n2, int d, int t)
{
    if (n1 < 1 || n2 < 1 || n1 >= kExMaxRows || n2 >= kExMaxRows || d < 1 || d > PLX_MAX_DIM || t < 1) return -1;
    return 4 * ex_work_floats(n1, n2, d, t);
}

extern "C" int plx_exact_splits(int64_t n1, int64_t n2, int d, int t)
{
    if (plx_exact_work_bytes(n1, n2, d, t) < 0) return -1;
    return ex_splits(n1, n2, d, t);
}

extern "C" int plx_exact_mvm(const float *d_x1, int64_t n1, const float *d_x2, int64_t n2, int d, int profile, const float *d_v,
                             int t, float *d_out, void *d_work, int64_t work_bytes, void *stream)
{
    PLX_TRY(ex_check("plx_exact_mvm", d_x1, n1, d_x2, n2, d, profile, d_v, d_v, t, d_out, d_work, work_bytes));
    return ex_run(false, d_x1, n1, d_x2, n2, d, profile, nullptr, d_v, t, d_out, d_work, stream);
}

extern "C" int plx_exact_grad(const float *d_x1, int64_t n1, const float *d_x2, int64_t n2, int d, int profile, const float *d_g,
                              const float *d_v, int t, float *d_grad_x1, void *d_work, int64_t work_bytes, void *stream)
{
    PLX_TRY(ex_check("plx_exact_grad", d_x1, n1, d_x2, n2, d, profile, d_g, d_v, t, d_grad_x1, d_work, work_bytes));
    return ex_run(true, d_x1, n1, d_x2, n2, d, profile, d_g, d_v, t, d_grad_x1, d_work, stream);
}
