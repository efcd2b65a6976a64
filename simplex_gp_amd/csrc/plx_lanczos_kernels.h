// plx_lanczos_kernels.h -- what a Lanczos step does next to its MVM (the variance cache of the reference's evaluation:
// gpytorch.settings.fast_pred_var + max_root_decomposition_size(lanc_iter), experiments/train_simplexgp.py:63-72, and
// training.PredictionCache for a double model): full re-orthogonalisation of w = A q_i against the basis q_0 .. q_i, the
// two recurrence coefficients, the next basis vector.  One templated source for fp32 and for double, instantiated by
// plx_lanczos.hip (float) and plx_lanczos_f64.hip (double), two translation units of a few lines each so that the two
// sets of kernels compile side by side.  With T = double every array and every operation is in double.
//
// In torch the step is ~19 launches (a gemv pair, a dot, a norm, a dozen element-wise and indexing kernels); at the
// sizes of the reference's UCI sets a launch is ~3.6 us of GPU time whatever it does (N = 10,623, d = 18: the MVM's own
// 21 launches take 75 us, the 19 around it 68 us).  Here it is four launches and two streams of the basis (what the gemv
// pair reads):
//
//   project           p0[g][j]  = sum over the rows of group g of Q[j][r] w[r]                       j = i - 1, i
//   subtract+project  c = sum_g p0[g];  w -= c_{i-1} Q[i-1] + c_i Q[i];  p1[g][j] = sum Q[j][r] w[r]     j <= i
//   subtract+norm     c2 = sum_g p1[g]; w -= sum_{j <= i} c2_j Q[j]; s[g] = sum w[r]^2;  alpha_i = c_i + c2_i
//   scale             beta_i = sqrt(sum_g s[g]);  Q[i+1] = w / max(beta_i, tiny)
//
// i.e. first the two directions in which w is large (the alpha q_i and beta q_{i-1} terms of the three-term recurrence),
// then one classical Gram-Schmidt pass against the whole basis.  The ORDER matters: a Gram-Schmidt pass leaves
// -E c in w (E = Q^T Q - I, c the coefficients it removed), so with the large coefficients alpha, beta still in w the
// departure of q_i from orthogonality to an early q_j is multiplied by alpha / beta_i per step -- measured in fp32 on a
// diagonal-plus-low-rank operator: |Q^T Q - I| = 0.77 after 40 steps with the full pass first, 4e-7 with the two large
// terms removed first (the torch form's order), 5e-7 with two full passes (a third stream of the basis).  So there is no
// second full pass, in either type.
//
// The contract: no atomics and no "last block" tickets.  Rows are split into at most LzScalar<T>::kMaxGroups groups of
// whole workgroup spans; every sum over groups is taken redundantly by each workgroup of the consuming launch in a fixed
// order, so the step is deterministic: two calls with the same arguments are bit-equal.
//
// Spans and groups.  A workgroup of 16 waves owns `span` consecutive rows and holds them in LDS (wv[span]), next to
// red[1024] (the sums over groups, the quarters of the short span) and c[256].  Small problems take many short spans (a
// launch is latency there, parallelism is what hides it: at span 256 the 16 waves share the basis rows of the projection
// and the four quarters of the workgroup share the j's of the subtraction); large ones at most kMaxGroups spans, so that
// the sums over groups stay a few KB per workgroup.
//   float:  spans 256 / 1024 / 4096 / 8192, each up to 256 groups; 8192 x 256 = 2,097,152 rows are served.
//   double: 8 span + 8 KiB + 2 KiB of static LDS.  A span of 8192 would be 64 KiB + 10 KiB, over the 64 KiB a workgroup's
//           static LDS allows; the span stops at 4096 (32 + 10 = 42 KiB, three workgroups of a CU's 160 KiB) and the group
//           limit rises to 512, so that the step serves the same 4096 x 512 = 2,097,152 rows.  Each workgroup of the two
//           subtracting launches re-reads groups x rows partial sums, groups^2 x rows x 8 bytes per launch against the
//           basis' n x rows x 8: a ratio of groups^2 / n = n / span^2.  The spans change where that ratio would pass 1
//           (256: n <= 65,536) or 1/2 (1024: n <= 524,288); at 4096 it is at most 1/8 (n = 2,097,152, i = 99:
//           512 x 512 x 100 x 8 = 210 MB of partials, each workgroup's 410 KB served from L2, against 2 x 1.68 GB of
//           basis from HBM).
// More rows than the last span x kMaxGroups: not served (plx_lanczos_work_floats / plx_lanczos_work_doubles < 0).
#pragma once
#include "plx_internal.h"

#include <algorithm>
#include <type_traits>

namespace plx {

constexpr int kLzMaxRows = 256;       // basis vectors a step can project on (the reference's lanc_iter default is 100)
constexpr int kLzThreads = 1024;

struct LzRung {
    int span;                         // rows per workgroup ...
    int64_t rows;                     // ... for n up to this many rows
};

struct LzShape {
    int span, groups;                 // groups > kMaxGroups: not served
};

// everything that differs between the two scalar types
template <typename T> struct LzScalar;
template <> struct LzScalar<float> {
    static constexpr int kMaxGroups = 256;
    static constexpr LzRung kLadder[] = {{256, 256 * 256}, {1024, 1024 * 256}, {4096, 4096 * 256}, {8192, 8192 * 256}};
    static constexpr const char *kStep = "plx_lanczos_step";
    static constexpr const char *kPlural = "floats";
    // q_{i+1} = w * (1 / max(beta, 1e-30))
    static __device__ __forceinline__ float guard(float beta) { return 1.f / fmaxf(beta, 1e-30f); }
    static __device__ __forceinline__ float scaled(float w, float g) { return w * g; }
};
template <> struct LzScalar<double> {
    static constexpr int kMaxGroups = 512;
    static constexpr LzRung kLadder[] = {{256, 256 * 256}, {1024, 1024 * 512}, {4096, 4096 * 512}};
    static constexpr const char *kStep = "plx_lanczos_step_f64";
    static constexpr const char *kPlural = "doubles";
    // q_{i+1} = w / max(beta, 1e-300)
    static __device__ __forceinline__ double guard(double beta) { return fmax(beta, 1e-300); }
    static __device__ __forceinline__ double scaled(double w, double g) { return w / g; }
};

template <typename T> constexpr int kLzRungs = sizeof(LzScalar<T>::kLadder) / sizeof(LzRung);
template <typename T> constexpr int kLzMaxSpan = LzScalar<T>::kLadder[kLzRungs<T> - 1].span;

// the 16-byte load of the wide subtraction: four floats or two doubles
template <typename T> constexpr int kLzPack = 16 / sizeof(T);
template <typename T> struct alignas(16) LzPack {
    T e[kLzPack<T>];
};

template <typename T>
static LzShape lz_shape(int64_t n)
{
    int k = 0;
    while (k + 1 < kLzRungs<T> && n > LzScalar<T>::kLadder[k].rows) ++k;
    LzShape s;
    s.span = LzScalar<T>::kLadder[k].span;
    s.groups = (int)std::min<int64_t>(1 << 30, std::max<int64_t>(1, ceil_div(n, (int64_t)s.span)));
    return s;
}

template <typename T>
__device__ __forceinline__ T lz_wave_sum(T a)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off);
    return a;
}

// c[j] = sum over g < groups of partial[g][j], first <= j < rows (0 elsewhere), in LDS; fixed order: the groups of a
// thread's slice strided (two chains), then the four slices in sequence.  red: kLzThreads elements of LDS.  Valid after the
// trailing barrier.
template <typename T>
__device__ __forceinline__ void lz_sum_groups(const T *__restrict__ partial, int groups, int first, int rows, T *red, T *c)
{
    constexpr int JW = kLzMaxRows;
    constexpr int SL = kLzThreads / JW;                     // 4 slices of the groups
    const int jj = threadIdx.x % JW, sl = threadIdx.x / JW;
    T a0 = T(0), a1 = T(0);
    if (jj >= first && jj < rows) {
        int g = sl;
        for (; g + SL < groups; g += 2 * SL) {
            const T p0 = partial[(size_t)g * kLzMaxRows + jj], p1 = partial[(size_t)(g + SL) * kLzMaxRows + jj];
            a0 += p0;
            a1 += p1;
        }
        if (g < groups) a0 += partial[(size_t)g * kLzMaxRows + jj];
    }
    red[threadIdx.x] = a0 + a1;
    __syncthreads();
    if ((int)threadIdx.x < JW) {
        T s = T(0);
#pragma unroll
        for (int k = 0; k < SL; ++k) s += red[k * JW + threadIdx.x];
        c[threadIdx.x] = ((int)threadIdx.x >= first && (int)threadIdx.x < rows) ? s : T(0);
    }
    __syncthreads();
}

// partial_out[j] = sum over this group's rows of Q[j][r] wv[r - r0]: a wave per basis row (strided), lanes across the
// group's rows (coalesced segments of 64 elements of the basis row), two basis rows in flight per wave
template <typename T, int SPAN>
__device__ __forceinline__ void lz_project(const T *__restrict__ Q, int64_t ld, int first, int rows, int64_t r0, int64_t n,
                                           const T *wv, T *__restrict__ partial_out)
{
    constexpr int W = kLzThreads / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lim = (int)min((int64_t)SPAN, n - r0);
    for (int j = first + wave; j < rows; j += 2 * W) {
        const T *qa = Q + (size_t)j * ld + r0;
        const bool two = j + W < rows;
        const T *qb = two ? qa + (size_t)W * ld : qa;
        T aa = T(0), ab = T(0);
#pragma unroll 4
        for (int r = lane; r < lim; r += 64) {
            const T x = wv[r];
            aa += qa[r] * x;
            ab += qb[r] * x;
        }
        aa = lz_wave_sum(aa);
        ab = lz_wave_sum(ab);
        if (lane == 0) {
            partial_out[j] = aa;
            if (two) partial_out[j + W] = ab;
        }
    }
}

// wv[r] -= sum over first <= j < rows of c[j] Q[j][r0 + r] for this group's rows; returns the sum of squares of the
// entries this thread wrote.  The loads of a batch of basis rows are issued together, branch-free (rows past n read a
// clamped, valid address and are dropped afterwards): with one predicated load per row in flight the pass ran at
// 2.2 TB/s at N = 1e6 in fp32, against 6 TB/s for the projection.  With P = 16 / sizeof(T) elements in a 16-byte piece:
//   SPAN >= P x 1024: thread t owns V = SPAN / (P x 1024) pieces of P consecutive rows per basis row (columns P t ..
//                 and the same + P x 1024), one 16-byte load each (ld % P == 0, d_q 16-byte aligned), U basis rows per
//                 batch: eight 16-byte loads in flight.  float: spans 4096 (V = 1, U = 8) and 8192 (V = 2, U = 4);
//                 double: span 4096 (V = 2, U = 4);
//   SPAN == 1024: thread t owns row t, eight basis rows per batch;
//   SPAN == 256:  the workgroup's four quarters share the j's of a row (j = first + quarter, + 4, ...) and meet in LDS
//                 (red: kLzThreads elements), summed in quarter order by the row's first thread.
template <typename T, int SPAN>
__device__ __forceinline__ T lz_subtract(const T *__restrict__ Q, int64_t ld, int first, int rows, int64_t r0, int64_t n,
                                         const T *c, T *wv, T *red, T *__restrict__ w)
{
    constexpr int P = kLzPack<T>;
    T ss = T(0);
    if constexpr (SPAN >= P * kLzThreads) {
        constexpr int V = SPAN / (P * kLzThreads);          // 16-byte pieces per thread and basis row: 1 or 2
        constexpr int U = V == 1 ? 8 : 4;                   // basis rows per batch
        LzPack<T> acc[V];
        int64_t off[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
#pragma unroll
            for (int e = 0; e < P; ++e) acc[v].e[e] = T(0);
            const int64_t col = r0 + P * ((int64_t)threadIdx.x + v * kLzThreads);
            off[v] = (col + (P - 1) < ld ? col : 0) / P;     // (a clamped piece is never used: its rows are >= n)
        }
        const LzPack<T> *qp = reinterpret_cast<const LzPack<T> *>(Q);
        const int64_t ldp = ld / P;
        int j = first;
        for (; j + U <= rows; j += U) {
            LzPack<T> x[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) x[u][v] = qp[(int64_t)(j + u) * ldp + off[v]];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const T cj = c[j + u];
#pragma unroll
                for (int v = 0; v < V; ++v)
#pragma unroll
                    for (int e = 0; e < P; ++e) acc[v].e[e] += cj * x[u][v].e[e];
            }
        }
        for (; j < rows; ++j) {
            const T cj = c[j];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const LzPack<T> x = qp[(int64_t)j * ldp + off[v]];
#pragma unroll
                for (int e = 0; e < P; ++e) acc[v].e[e] += cj * x.e[e];
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int r = P * (threadIdx.x + v * kLzThreads);
#pragma unroll
            for (int e = 0; e < P; ++e)
                if (r0 + r + e < n) {
                    const T val = wv[r + e] - acc[v].e[e];
                    wv[r + e] = val;
                    w[r0 + r + e] = val;
                    ss += val * val;
                }
        }
    } else {
        constexpr int JS = kLzThreads / SPAN;               // 1 (SPAN 1024) or 4 (SPAN 256)
        constexpr int U = 8;
        const int r = threadIdx.x % SPAN, js = threadIdx.x / SPAN;
        const bool ok = r0 + r < n;
        const T *q = Q + (ok ? r0 + r : 0);
        T acc = T(0);
        int j = first + js;
        for (; j + (U - 1) * JS < rows; j += U * JS) {
            T x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = q[(int64_t)(j + u * JS) * ld];
#pragma unroll
            for (int u = 0; u < U; ++u) acc += c[j + u * JS] * x[u];
        }
        for (; j < rows; j += JS) acc += c[j] * q[(int64_t)j * ld];
        if constexpr (JS > 1) {
            red[threadIdx.x] = acc;
            __syncthreads();
            acc = T(0);
            if (js == 0) {
#pragma unroll
                for (int k = 0; k < JS; ++k) acc += red[k * SPAN + r];
            }
        }
        if (js == 0 && ok) {
            const T val = wv[r] - acc;
            wv[r] = val;
            w[r0 + r] = val;
            ss = val * val;
        }
    }
    return ss;
}

template <typename T, int SPAN>
__device__ __forceinline__ void lz_stage(const T *__restrict__ w, int64_t r0, int64_t n, T *wv)
{
    for (int r = threadIdx.x; r < SPAN; r += kLzThreads) wv[r] = r0 + r < n ? w[r0 + r] : T(0);
    __syncthreads();
}

template <typename T, int SPAN>
__global__ __launch_bounds__(kLzThreads) void lanczos_project_kernel(const T *__restrict__ Q, int64_t ld, const T *__restrict__ w,
                                                                     int64_t n, int rows, T *__restrict__ partial)
{
    __shared__ T wv[SPAN];
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    lz_stage<T, SPAN>(w, r0, n, wv);
    lz_project<T, SPAN>(Q, ld, max(0, rows - 2), rows, r0, n, wv, partial + (size_t)blockIdx.x * kLzMaxRows);
}

template <typename T, int SPAN>
__global__ __launch_bounds__(kLzThreads) void lanczos_subtract_project_kernel(const T *__restrict__ Q, int64_t ld,
                                                                              T *__restrict__ w, int64_t n, int rows,
                                                                              const T *__restrict__ partial_in, int groups,
                                                                              T *__restrict__ partial_out, T *__restrict__ c_out)
{
    __shared__ T wv[SPAN];
    __shared__ T red[kLzThreads];
    __shared__ T c[kLzMaxRows];
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    const int first = max(0, rows - 2);
    lz_sum_groups<T>(partial_in, groups, first, rows, red, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) c_out[0] = c[rows - 1];          // the first part of alpha_i
    lz_stage<T, SPAN>(w, r0, n, wv);
    lz_subtract<T, SPAN>(Q, ld, first, rows, r0, n, c, wv, red, w);
    __syncthreads();
    lz_project<T, SPAN>(Q, ld, 0, rows, r0, n, wv, partial_out + (size_t)blockIdx.x * kLzMaxRows);
}

template <typename T, int SPAN>
__global__ __launch_bounds__(kLzThreads) void lanczos_subtract_norm_kernel(const T *__restrict__ Q, int64_t ld, T *__restrict__ w,
                                                                           int64_t n, int rows, const T *__restrict__ partial_in,
                                                                           int groups, const T *__restrict__ c_first,
                                                                           T *__restrict__ alphas, T *__restrict__ sumsq)
{
    __shared__ T wv[SPAN];
    __shared__ T red[kLzThreads];
    __shared__ T c[kLzMaxRows];
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    lz_sum_groups<T>(partial_in, groups, 0, rows, red, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) alphas[rows - 1] = c_first[0] + c[rows - 1];
    lz_stage<T, SPAN>(w, r0, n, wv);
    T ss = lz_subtract<T, SPAN>(Q, ld, 0, rows, r0, n, c, wv, red, w);
    // sum of squares of the group: within the waves, then the waves in sequence
    const T ws = lz_wave_sum(ss);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        T s = T(0);
        for (int k = 0; k < kLzThreads / 64; ++k) s += red[k];
        sumsq[blockIdx.x] = s;
    }
}

// beta = sqrt(sum over the groups of sumsq[g]), taken by every workgroup (the same order in every workgroup and every
// call), and Q[i+1] = w scaled by the type's guard.  The sum is the one place with a body per type: merging the two would
// change the rounding of beta and of every entry of q_{i+1} in one precision -- a change of results, not of form.
//   float:  thread 0 sums the groups in sequence out of LDS;
//   double: the first wave, lane l taking groups l, l + 64, ... in order, then the lanes meet in a butterfly.
template <typename T, int SPAN>
__global__ __launch_bounds__(kLzThreads) void lanczos_scale_kernel(const T *__restrict__ w, int64_t n, const T *__restrict__ sumsq,
                                                                   int groups, T *__restrict__ qnext, T *__restrict__ betas, int i)
{
    using S = LzScalar<T>;
    __shared__ T guard_s;
    if constexpr (std::is_same_v<T, float>) {
        __shared__ T red[S::kMaxGroups];
        if ((int)threadIdx.x < S::kMaxGroups) red[threadIdx.x] = (int)threadIdx.x < groups ? sumsq[threadIdx.x] : T(0);
        __syncthreads();
        if (threadIdx.x == 0) {
            T s = T(0);
            for (int g = 0; g < groups; ++g) s += red[g];
            const T beta = sqrtf(s);
            guard_s = S::guard(beta);
            if (blockIdx.x == 0) betas[i] = beta;
        }
    } else {
        if (threadIdx.x < 64) {
            T s = T(0);
            for (int g = threadIdx.x; g < groups; g += 64) s += sumsq[g];
            s = lz_wave_sum(s);
            if (threadIdx.x == 0) {
                const T beta = sqrt(s);
                guard_s = S::guard(beta);
                if (blockIdx.x == 0) betas[i] = beta;
            }
        }
    }
    __syncthreads();
    const T g = guard_s;
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    for (int k = threadIdx.x; k < SPAN; k += kLzThreads)
        if (r0 + k < n) qnext[r0 + k] = S::scaled(w[r0 + k], g);
}

// work: p0 [kMaxGroups][kLzMaxRows], p1 the same, c0 [kLzMaxRows], sumsq [kMaxGroups]
template <typename T>
static int64_t lz_work_count(int64_t n)
{
    constexpr int64_t G = LzScalar<T>::kMaxGroups;
    if (n < 1 || lz_shape<T>(n).groups > G) return -1;
    return 2 * G * kLzMaxRows + kLzMaxRows + G;
}

template <typename T, int SPAN>
static void lanczos_launch(T *Q, int64_t ld, T *w, int64_t n, int i, T *alphas, T *betas, T *work, int groups, hipStream_t s)
{
    constexpr size_t G = LzScalar<T>::kMaxGroups;
    T *p0 = work, *p1 = work + G * kLzMaxRows, *c0 = p1 + G * kLzMaxRows, *sumsq = c0 + kLzMaxRows;
    const int rows = i + 1;
    lanczos_project_kernel<T, SPAN><<<groups, kLzThreads, 0, s>>>(Q, ld, w, n, rows, p0);
    lanczos_subtract_project_kernel<T, SPAN><<<groups, kLzThreads, 0, s>>>(Q, ld, w, n, rows, p0, groups, p1, c0);
    lanczos_subtract_norm_kernel<T, SPAN><<<groups, kLzThreads, 0, s>>>(Q, ld, w, n, rows, p1, groups, c0, alphas, sumsq);
    lanczos_scale_kernel<T, SPAN><<<groups, kLzThreads, 0, s>>>(w, n, sumsq, groups, Q + (size_t)(i + 1) * ld, betas, i);
}

// the launcher of `span`: rung K of the type's ladder or a later one, so only the spans of kLadder are instantiated
template <typename T, int K = 0>
static void lz_dispatch(int span, T *Q, int64_t ld, T *w, int64_t n, int i, T *alphas, T *betas, T *work, int groups, hipStream_t s)
{
    constexpr int SPAN = LzScalar<T>::kLadder[K].span;
    if constexpr (K + 1 < kLzRungs<T>) {
        if (span != SPAN) return lz_dispatch<T, K + 1>(span, Q, ld, w, n, i, alphas, betas, work, groups, s);
    }
    lanczos_launch<T, SPAN>(Q, ld, w, n, i, alphas, betas, work, groups, s);
}

// plx_lanczos_step / plx_lanczos_step_f64: every check before any GPU work, then the four launches
template <typename T>
static int lz_step(T *d_q, int64_t ld, T *d_w, int64_t n, int i, T *d_alphas, T *d_betas, T *d_work, void *stream)
{
    using S = LzScalar<T>;
    constexpr int P = kLzPack<T>;
    static_assert(S::kLadder[kLzRungs<T> - 1].rows == (int64_t)S::kMaxGroups * kLzMaxSpan<T>, "the last rung ends at the group limit");
    const char *who = S::kStep;
    if (!d_q || !d_w || !d_alphas || !d_betas || !d_work) {
        set_error("%s: NULL argument", who);
        return PLX_ERR_INVALID;
    }
    const uintptr_t bits = (uintptr_t)d_q | (uintptr_t)d_w | (uintptr_t)d_alphas | (uintptr_t)d_betas | (uintptr_t)d_work;
    if ((bits & (sizeof(T) - 1)) != 0) {
        set_error("%s: buffers of %s must be %d-byte aligned", who, S::kPlural, (int)sizeof(T));
        return PLX_ERR_INVALID;
    }
    if (n < 1 || ld < n || i < 0 || i + 1 > kLzMaxRows) {
        set_error("%s: n = %lld, ld = %lld, step %d (n >= 1, ld >= n, at most %d basis vectors)", who, (long long)n, (long long)ld, i,
                  kLzMaxRows);
        return PLX_ERR_INVALID;
    }
    if (ld % P != 0 || ((uintptr_t)d_q & 15) != 0) {
        set_error("%s: the basis must be 16-byte aligned with ld a multiple of %d (ld = %lld)", who, P, (long long)ld);
        return PLX_ERR_INVALID;
    }
    const LzShape sh = lz_shape<T>(n);
    if (sh.groups > S::kMaxGroups) {
        set_error("%s: n = %lld is more than %lld rows", who, (long long)n, (long long)S::kMaxGroups * kLzMaxSpan<T>);
        return PLX_ERR_INVALID;
    }
    // w is read and written while rows 0..i of the basis are read and row i + 1 is written: no part of it inside them
    if (d_w < d_q + (size_t)(i + 2) * ld && d_w + n > d_q) {
        set_error("%s: d_w overlaps rows 0..%d of the basis", who, i + 1);
        return PLX_ERR_INVALID;
    }
    lz_dispatch<T>(sh.span, d_q, ld, d_w, n, i, d_alphas, d_betas, d_work, sh.groups, (hipStream_t)stream);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
