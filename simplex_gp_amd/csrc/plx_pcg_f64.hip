// plx_pcg_f64.hip -- the float64 application of the pivoted-Cholesky preconditioner next to the float64 CG solve
// (include/plx.h: plx_pcg_gram_f64, plx_pcg_project_f64, plx_pcg_apply_f64, plx_pcg_step_direction_f64,
// plx_pcg_work_doubles).
//
// The factor is the one plx_pchol_* builds and stays stored in fp32, L^T row-major [kp][ld] (plx_pcg.hip's layout: kp a
// multiple of 16, ld a multiple of 64, zero tails); an fp32 entry converts to double exactly, so P = L L^T + sigma^2 I is
// the same matrix here as anywhere else the factor appears.  Only its APPLICATION is in double:
//   pcg64_gram_kernel     per-workgroup partials of G = L^T R on v_mfma_f64_16x16x4_f64: exact products of the converted
//                         entries (24 x 53 bits is rounded once, by the fma), fp64 accumulation
//   pcg64_project_kernel  the partials in workgroup order, then (plx_pcg_project_f64) T = C^-1 G with C^-1 fp64 [kp][kp]
//   pcg64_apply_kernel    Z = (in_scale R - L T) out_scale, one row per lane, and the workgroup's partial <R, Z>
// <R, Z> is summed from the apply partials by coldot_final, and plx_pcg_step_direction_f64 (beta = rz' / rz, P = Z + beta P,
// active' from the TRUE residual norm) is cg_step_direction: plx_cg_kernels.h with T = double, instantiated by plx_cg_f64.hip.
// Vectors are double [n][t], rows in whatever order the factor's n dimension is in (solvers.LatticePreconditioner64 keeps
// both in the caller's order, like every fp64 call).  No atomics: partial sums per workgroup, fixed-order final sums.
#include "plx_internal.h"

#include <algorithm>

namespace plx {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGram64Blocks = 512;    // most workgroups of the gram kernel = partial sums per (j, c); the work buffer is sized for it
constexpr int kPcg64Cols = 16;        // column tile: the N of the 16x16x4 MFMA; G and T are [kp][16]

// ---- G = L^T R ---------------------------------------------------------------------------------------------------
// pcg_gram_kernel's tile walk: one wave per 64-row tile, lane l loads the 16 bytes lt[j][i0 + 16 s + 4 (l >> 4) .. + 3]
// (s = 0..3), component q of that load is the A operand of MFMA (s, q), whose B operand is R[i0 + 16 s + 4 (l >> 4) + q]
// [l & 15].  v_mfma_f64_16x16x4_f64 takes A[j = lane & 15][k = lane >> 4] and B[k = lane >> 4][c = lane & 15] like the
// f32 form; its result is D[j = (lane >> 4) + 4 reg][c = lane & 15] (the f32 form: 4 (lane >> 4) + reg).
template <int JT>
__global__ __launch_bounds__(kBlock) void pcg64_gram_kernel(const float *__restrict__ lt, int64_t ld, int kp, int j0,
                                                            const double *__restrict__ R, int64_t n, int t, int ntiles,
                                                            double *__restrict__ partial)
{
    __shared__ double red[JT * 16 * kPcg64Cols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    f64x4 acc[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) acc[jt] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int wstride = gridDim.x * (kBlock / 64);
    for (int tile = blockIdx.x * (kBlock / 64) + wave; tile < ntiles; tile += wstride) {
        const int64_t i0 = (int64_t)tile * 64;
        // every factor load of the tile is issued before the first MFMA (the tile's columns i0 .. i0 + 63 are inside ld)
        float4 araw[JT][4];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const float *row = lt + (int64_t)(j0 + 16 * jt + lr) * ld + i0 + 4 * lk;
#pragma unroll
            for (int s = 0; s < 4; ++s) araw[jt][s] = *reinterpret_cast<const float4 *>(row + 16 * s);
        }
        double b[16];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t i = i0 + 16 * s + 4 * lk + q;
                b[4 * s + q] = (lr < t && i < n) ? R[i * t + lr] : 0.0;
            }
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float4 v = araw[jt][s];
                const double a[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[4 * s + q], acc[jt], 0, 0, 0);
            }
    }
    // the four waves add into one LDS image in wave order (fixed summation order)
    for (int w = 0; w < kBlock / 64; ++w) {
        if (wave == w) {
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int idx = (jt * 16 + lk + 4 * e) * kPcg64Cols + lr;
                    red[idx] = (w == 0 ? 0.0 : red[idx]) + acc[jt][e];
                }
        }
        __syncthreads();
    }
    // partial[workgroup][c][j]: consecutive threads write consecutive j
    for (int x = threadIdx.x; x < JT * 16 * kPcg64Cols; x += kBlock) {
        const int jj = x % (JT * 16), c = x / (JT * 16);
        partial[((size_t)blockIdx.x * kPcg64Cols + c) * kp + j0 + jj] = red[jj * kPcg64Cols + c];
    }
}

// ---- one workgroup per column: g = the partials in workgroup order; PROJECT: out = C^-1 g (C^-1 symmetric: its column j
// is read as row j, consecutive threads consecutive addresses), else out = g.  pcg_project_kernel in double throughout:
// thread (j, q) takes the terms q, q + groups, ... of entry j, then the groups are added in order. ----------------------
template <bool PROJECT>
__global__ __launch_bounds__(1024) void pcg64_project_kernel(const double *__restrict__ partial, int nparts, int kp,
                                                             const double *__restrict__ cinv, double *__restrict__ out)
{
    extern __shared__ double sm[];          // g[kp] | grp[groups][kp]
    double *g = sm, *grp = sm + kp;
    const int c = blockIdx.x;
    const int groups = max(1, (int)blockDim.x / kp);
    const int j = threadIdx.x % kp, q = threadIdx.x / kp;
    if (q < groups) {
        double s = 0.0;
        int w = q;
        for (; w + 7 * groups < nparts; w += 8 * groups) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[((size_t)(w + u * groups) * kPcg64Cols + c) * kp + j];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; w < nparts; w += groups) s += partial[((size_t)w * kPcg64Cols + c) * kp + j];
        grp[q * kp + j] = s;
    }
    __syncthreads();
    for (int jj = threadIdx.x; jj < kp; jj += blockDim.x) {
        double s = 0.0;
        for (int qq = 0; qq < groups; ++qq) s += grp[qq * kp + jj];
        if constexpr (PROJECT) g[jj] = s;
        else out[jj * kPcg64Cols + c] = s;
    }
    if constexpr (PROJECT) {
        __syncthreads();
        if (q < groups) {
            double s = 0.0;
            int qq = q;
            for (; qq + 3 * groups < kp; qq += 4 * groups) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = cinv[(size_t)(qq + u * groups) * kp + j];
#pragma unroll
                for (int u = 0; u < 4; ++u) s += v[u] * g[qq + u * groups];
            }
            for (; qq < kp; qq += groups) s += cinv[(size_t)qq * kp + j] * g[qq];
            grp[q * kp + j] = s;
        }
        __syncthreads();
        for (int jj = threadIdx.x; jj < kp; jj += blockDim.x) {
            double s = 0.0;
            for (int qq = 0; qq < groups; ++qq) s += grp[qq * kp + jj];
            out[jj * kPcg64Cols + c] = s;
        }
    }
}

// ---- Z = (in_scale R - L T) out_scale, one row per lane: the k rows of L^T stream through coalesced, the k x T
// coefficients are wave-uniform.  VEC: rows of R and Z as double2 (T even, both 16-byte aligned).  The workgroup's
// partial <R, Z> per column comes from the same registers. ---------------------------------------------------------------
template <int T, bool VEC>
__global__ __launch_bounds__(kBlock) void pcg64_apply_kernel(const float *__restrict__ lt, int64_t ld, int k,
                                                             const double *__restrict__ R, int64_t n,
                                                             const double *__restrict__ Tm, const double *__restrict__ scal,
                                                             double *__restrict__ Z, double *__restrict__ partial)
{
    static_assert(!VEC || T % 2 == 0, "double2 rows need an even column count");
    __shared__ double red[(kBlock / 64) * T];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc[T];
#pragma unroll
    for (int c = 0; c < T; ++c) acc[c] = 0.0;
    // (rows beyond n read the zero tail of the factor, rows beyond ld its first column: neither is stored)
    const int64_t ic = i < ld ? i : 0;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
        const double l = (double)lt[(int64_t)j * ld + ic];
        const double *tr = Tm + j * kPcg64Cols;
#pragma unroll
        for (int c = 0; c < T; ++c) acc[c] = fma(l, tr[c], acc[c]);
    }
    const double in_scale = scal[0], out_scale = scal[1];
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;
    double rv[T], z[T], dot[T];
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < T / 2; ++q) {
            const double2 v = reinterpret_cast<const double2 *>(R + ii * T)[q];
            rv[2 * q] = v.x; rv[2 * q + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < T; ++c) rv[c] = R[ii * T + c];
    }
#pragma unroll
    for (int c = 0; c < T; ++c) {
        z[c] = (rv[c] * in_scale - acc[c]) * out_scale;
        dot[c] = live ? rv[c] * z[c] : 0.0;
    }
    if (live) {
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < T / 2; ++q) reinterpret_cast<double2 *>(Z + i * T)[q] = make_double2(z[2 * q], z[2 * q + 1]);
        } else {
#pragma unroll
            for (int c = 0; c < T; ++c) Z[i * T + c] = z[c];
        }
    }
    // <R, Z> per column: lanes of a wave by a fixed xor tree, the four waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < T; ++c) {
        double p = dot[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
        if (lane == 0) red[wave * T + c] = p;
    }
    __syncthreads();
    if ((int)threadIdx.x < T) {
        double s = 0.0;
        for (int w = 0; w < kBlock / 64; ++w) s += red[w * T + threadIdx.x];
        partial[(size_t)blockIdx.x * T + threadIdx.x] = s;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// workgroups of the gram kernel = partial rows the final sum walks: one per four tiles (a wave each) up to kGram64Blocks
static int gram64_parts(int64_t n) { return (int)std::min<int64_t>(kGram64Blocks, ceil_div(ceil_div(n, 64), kBlock / 64)); }

// work layout (doubles): gram partials | apply partials
static size_t pcg64_gram_doubles(int kp) { return (size_t)kGram64Blocks * kPcg64Cols * kp; }

static int gram64_launch(const float *lt, int64_t ld, int kp, const double *R, int64_t n, int t, double *partial, hipStream_t s)
{
    const int ntiles = ceil_div(n, 64), parts = gram64_parts(n);
    for (int j0 = 0; j0 < kp; j0 += 128) {
        const int jt = std::min(8, (kp - j0) / 16);
        switch (jt) {
#define PLX_GRAM64_CASE(J) case J: pcg64_gram_kernel<J><<<parts, kBlock, 0, s>>>(lt, ld, kp, j0, R, n, t, ntiles, partial); break;
        PLX_GRAM64_CASE(1) PLX_GRAM64_CASE(2) PLX_GRAM64_CASE(3) PLX_GRAM64_CASE(4)
        PLX_GRAM64_CASE(5) PLX_GRAM64_CASE(6) PLX_GRAM64_CASE(7) PLX_GRAM64_CASE(8)
#undef PLX_GRAM64_CASE
        }
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <bool VEC>
static int apply64_launch(const float *lt, int64_t ld, int k, const double *R, int64_t n, int t, const double *Tm,
                          const double *scal, double *Z, double *partial, hipStream_t s)
{
    const int grid = ceil_div(n, kBlock);
    switch (t) {
#define PLX_APPLY64_CASE(T) case T: pcg64_apply_kernel<T, VEC && T % 2 == 0><<<grid, kBlock, 0, s>>>(lt, ld, k, R, n, Tm, scal, Z, partial); break;
    PLX_APPLY64_CASE(1) PLX_APPLY64_CASE(2) PLX_APPLY64_CASE(3) PLX_APPLY64_CASE(4) PLX_APPLY64_CASE(5) PLX_APPLY64_CASE(6)
    PLX_APPLY64_CASE(7) PLX_APPLY64_CASE(8) PLX_APPLY64_CASE(9) PLX_APPLY64_CASE(10) PLX_APPLY64_CASE(11) PLX_APPLY64_CASE(12)
    PLX_APPLY64_CASE(13) PLX_APPLY64_CASE(14) PLX_APPLY64_CASE(15) PLX_APPLY64_CASE(16)
#undef PLX_APPLY64_CASE
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

// Everything a factor call checks before any launch: the factor's shape contract (plx_pcg.hip: factor_shape_ok), then
// every other pointer (non-NULL, 8-byte aligned).
static int check_pcg64(const char *who, const void *lt, int64_t ld, int kp, int64_t n, int t,
                       std::initializer_list<const void *> ptrs)
{
    if (!lt) { set_error("%s: NULL factor", who); return PLX_ERR_INVALID; }
    if (n < 1 || ld < n || (ld & 63) || kp < 16 || (kp & 15) || kp > 1024 || t < 1 || t > kPcg64Cols) {
        set_error("%s: n = %lld, ld = %lld (a multiple of 64, >= n), kp = %d (a multiple of 16, <= 1024), %d columns (1..16)",
                  who, (long long)n, (long long)ld, kp, t);
        return PLX_ERR_INVALID;
    }
    if ((reinterpret_cast<uintptr_t>(lt) & 15) != 0) { set_error("%s: the factor must be 16-byte aligned", who); return PLX_ERR_INVALID; }
    return cg_check(cg_rules_f64(who), ptrs, n, t);      // (n and t are inside its ranges by now: the pointer checks remain)
}

}  // namespace plx

using namespace plx;

extern "C" int64_t plx_pcg_work_doubles(int64_t n, int kp, int t)
{
    if (n < 1 || kp < 16 || (kp & 15) || kp > 1024 || t < 1 || t > kPcg64Cols) return -1;
    return (int64_t)pcg64_gram_doubles(kp) + (int64_t)ceil_div(n, kBlock) * kPcg64Cols;
}

extern "C" int plx_pcg_gram_f64(const float *d_lt, int64_t ld, int kp, const double *d_r, int64_t n, int t, double *d_g,
                                double *d_work, void *stream)
{
    PLX_TRY(check_pcg64("plx_pcg_gram_f64", d_lt, ld, kp, n, t, {d_r, d_g, d_work}));
    hipStream_t s = (hipStream_t)stream;
    PLX_TRY(gram64_launch(d_lt, ld, kp, d_r, n, t, d_work, s));
    const int groups = std::max(1, 1024 / kp);
    pcg64_project_kernel<false><<<t, 1024, (size_t)kp * (1 + groups) * sizeof(double), s>>>(d_work, gram64_parts(n), kp, nullptr, d_g);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

extern "C" int plx_pcg_project_f64(const float *d_lt, int64_t ld, int kp, const double *d_r, int64_t n, int t,
                                   const double *d_cinv, double *d_t, double *d_work, void *stream)
{
    PLX_TRY(check_pcg64("plx_pcg_project_f64", d_lt, ld, kp, n, t, {d_r, d_cinv, d_t, d_work}));
    hipStream_t s = (hipStream_t)stream;
    PLX_TRY(gram64_launch(d_lt, ld, kp, d_r, n, t, d_work, s));
    const int groups = std::max(1, 1024 / kp);
    pcg64_project_kernel<true><<<t, 1024, (size_t)kp * (1 + groups) * sizeof(double), s>>>(d_work, gram64_parts(n), kp, d_cinv, d_t);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

extern "C" int plx_pcg_apply_f64(const float *d_lt, int64_t ld, int kp, int k, const double *d_r, int64_t n, int t,
                                 const double *d_t, const double *d_scale, double *d_z, double *d_rz, double *d_work,
                                 void *stream)
{
    PLX_TRY(check_pcg64("plx_pcg_apply_f64", d_lt, ld, kp, n, t, {d_r, d_t, d_scale, d_z, d_work}));
    if ((reinterpret_cast<uintptr_t>(d_rz) & 7) != 0) { set_error("plx_pcg_apply_f64: buffers of doubles must be 8-byte aligned"); return PLX_ERR_INVALID; }
    if (k < 0 || k > kp) { set_error("plx_pcg_apply_f64: k = %d outside 0..kp", k); return PLX_ERR_INVALID; }
    if (d_z == d_r) { set_error("plx_pcg_apply_f64: Z and R must be different buffers"); return PLX_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    double *part = d_work + pcg64_gram_doubles(kp);
    const bool vec = ((reinterpret_cast<uintptr_t>(d_r) | reinterpret_cast<uintptr_t>(d_z)) & 15) == 0;
    if (vec) PLX_TRY(apply64_launch<true>(d_lt, ld, k, d_r, n, t, d_t, d_scale, d_z, part, s));
    else PLX_TRY(apply64_launch<false>(d_lt, ld, k, d_r, n, t, d_t, d_scale, d_z, part, s));
    if (d_rz) PLX_TRY(coldot_final(part, ceil_div(n, kBlock), t, t, d_rz, s));
    return PLX_OK;
}

extern "C" int plx_pcg_step_direction_f64(double *d_p, const double *d_z, const double *d_rz_new, const double *d_rz,
                                          const double *d_rr, const double *d_active, const double *d_b_norm, double tol,
                                          int64_t n, int vd, double *d_beta, double *d_active_out, void *stream)
{
    return cg_step_direction(cg_rules_f64("plx_pcg_step_direction_f64"), d_p, d_z, d_rz_new, d_rz, d_rr, d_active, d_b_norm, tol,
                             n, vd, d_beta, d_active_out, (hipStream_t)stream);
}
