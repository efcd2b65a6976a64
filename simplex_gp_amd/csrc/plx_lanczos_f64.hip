// plx_lanczos_f64.hip -- the Lanczos step of plx_lanczos.hip with every array in double: what a double model's variance
// cache (training.PredictionCache) does next to its MVM.  The recurrence and its ORDER are those of plx_lanczos.hip (its
// header records why the two large components go first: a Gram-Schmidt pass leaves -E c in w):
//
//   project           p0[g][j]  = sum over the rows of group g of Q[j][r] w[r]                       j = i - 1, i
//   subtract+project  c = sum_g p0[g];  w -= c_{i-1} Q[i-1] + c_i Q[i];  p1[g][j] = sum Q[j][r] w[r]     j <= i
//   subtract+norm     c2 = sum_g p1[g]; w -= sum_{j <= i} c2_j Q[j]; s[g] = sum w[r]^2;  alpha_i = c_i + c2_i
//   scale             beta_i = sqrt(sum_g s[g]);  Q[i+1] = w / max(beta_i, 1e-300)
//
// Four launches, two streams of the basis, no atomics and no "last block" tickets: every sum over groups is taken
// redundantly by each workgroup of the consuming launch in a fixed order, so two calls with the same arguments are
// bit-equal.  No second full Gram-Schmidt pass (a third stream of the basis), as in fp32.
//
// Spans and groups.  A workgroup of 16 waves owns `span` consecutive rows and holds them in LDS (wv[span] doubles), next to
// red[1024] (the sums over groups, the quarters of the short span) and c[256]: 8 span + 8 KiB + 2 KiB of static LDS.  The
// fp32 step's span of 8192 would be 64 KiB + 10 KiB, over the 64 KiB a workgroup's static LDS allows; the span here stops
// at 4096 (32 + 10 = 42 KiB, three workgroups of a CU's 160 KiB) and the group limit rises to 512, so that the step
// serves the same 4096 x 512 = 2,097,152 rows.  Each workgroup of the two subtracting launches re-reads groups x rows
// partial sums, groups^2 x rows x 8 bytes per launch against the basis' n x rows x 8: a ratio of groups^2 / n =
// n / span^2.  The spans change where that ratio would pass 1 (256: n <= 65,536) or 1/2 (1024: n <= 524,288); at 4096 it
// is at most 1/8 (n = 2,097,152, i = 99: 512 x 512 x 100 x 8 = 210 MB of partials, each workgroup's 410 KB served from
// L2, against 2 x 1.68 GB of basis from HBM).
#include "plx_internal.h"

#include <algorithm>

namespace plx {

constexpr int kLz64MaxRows = 256;     // = plx_lanczos_max_rows()
constexpr int kLz64MaxGroups = 512;
constexpr int kLz64MaxSpan = 4096;
constexpr int kLz64Threads = 1024;

struct Lz64Shape {
    int span, groups;                 // groups > kLz64MaxGroups: not served
};

static Lz64Shape lanczos64_shape(int64_t n)
{
    Lz64Shape s;
    if (n <= 256 * (int64_t)256) s.span = 256;                         // n / span^2 <= 1
    else if (n <= 1024 * (int64_t)kLz64MaxGroups) s.span = 1024;       // <= 1/2
    else s.span = kLz64MaxSpan;
    s.groups = (int)std::min<int64_t>(1 << 30, std::max<int64_t>(1, ceil_div(n, (int64_t)s.span)));
    return s;
}

__device__ __forceinline__ double lz64_wave_sum(double a)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off);
    return a;
}

// c[j] = sum over g < groups of partial[g][j], first <= j < rows (0 elsewhere), in LDS; fixed order: the groups of a
// thread's slice strided (two chains), then the four slices in sequence.  red: kLz64Threads doubles of LDS.  Valid after the
// trailing barrier.
__device__ __forceinline__ void lz64_sum_groups(const double *__restrict__ partial, int groups, int first, int rows, double *red,
                                                double *c)
{
    constexpr int JW = kLz64MaxRows;
    constexpr int SL = kLz64Threads / JW;                   // 4 slices of the groups
    const int jj = threadIdx.x % JW, sl = threadIdx.x / JW;
    double a0 = 0.0, a1 = 0.0;
    if (jj >= first && jj < rows) {
        int g = sl;
        for (; g + SL < groups; g += 2 * SL) {
            const double p0 = partial[(size_t)g * kLz64MaxRows + jj], p1 = partial[(size_t)(g + SL) * kLz64MaxRows + jj];
            a0 += p0;
            a1 += p1;
        }
        if (g < groups) a0 += partial[(size_t)g * kLz64MaxRows + jj];
    }
    red[threadIdx.x] = a0 + a1;
    __syncthreads();
    if ((int)threadIdx.x < JW) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < SL; ++k) s += red[k * JW + threadIdx.x];
        c[threadIdx.x] = ((int)threadIdx.x >= first && (int)threadIdx.x < rows) ? s : 0.0;
    }
    __syncthreads();
}

// partial_out[j] = sum over this group's rows of Q[j][r] wv[r - r0]: a wave per basis row (strided), lanes across the
// group's rows (coalesced 512-byte segments of the basis row), two basis rows in flight per wave
template <int SPAN>
__device__ __forceinline__ void lz64_project(const double *__restrict__ Q, int64_t ld, int first, int rows, int64_t r0, int64_t n,
                                             const double *wv, double *__restrict__ partial_out)
{
    constexpr int W = kLz64Threads / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lim = (int)min((int64_t)SPAN, n - r0);
    for (int j = first + wave; j < rows; j += 2 * W) {
        const double *qa = Q + (size_t)j * ld + r0;
        const bool two = j + W < rows;
        const double *qb = two ? qa + (size_t)W * ld : qa;
        double aa = 0.0, ab = 0.0;
#pragma unroll 4
        for (int r = lane; r < lim; r += 64) {
            const double x = wv[r];
            aa += qa[r] * x;
            ab += qb[r] * x;
        }
        aa = lz64_wave_sum(aa);
        ab = lz64_wave_sum(ab);
        if (lane == 0) {
            partial_out[j] = aa;
            if (two) partial_out[j + W] = ab;
        }
    }
}

// wv[r] -= sum over first <= j < rows of c[j] Q[j][r0 + r] for this group's rows; returns the sum of squares of the
// entries this thread wrote.  The loads of a batch of basis rows are issued together, branch-free (rows past n read a
// clamped, valid address and are dropped afterwards; plx_lanczos.hip's lz_subtract records what one predicated load in
// flight cost).
//   SPAN == 4096: thread t owns two 16-byte pieces (2 doubles each: columns 2 t, 2 t + 1 and the same + 2048) per basis
//                 row, four basis rows per batch: eight 16-byte loads in flight (ld % 2 == 0, d_q 16-byte aligned);
//   SPAN == 1024: thread t owns row t, eight basis rows per batch;
//   SPAN == 256:  the workgroup's four quarters share the j's of a row (j = first + quarter, + 4, ...) and meet in LDS
//                 (red: kLz64Threads doubles), summed in quarter order by the row's first thread.
template <int SPAN>
__device__ __forceinline__ double lz64_subtract(const double *__restrict__ Q, int64_t ld, int first, int rows, int64_t r0, int64_t n,
                                                const double *c, double *wv, double *red, double *__restrict__ w)
{
    double ss = 0.0;
    if constexpr (SPAN >= 2048) {
        constexpr int V = SPAN / (2 * kLz64Threads);        // 16-byte pieces per thread and basis row: 2
        constexpr int U = 4;                                // basis rows per batch
        double2 acc[V];
        int64_t off[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            acc[v] = make_double2(0.0, 0.0);
            const int64_t col = r0 + 2 * ((int64_t)threadIdx.x + v * kLz64Threads);
            off[v] = (col + 1 < ld ? col : 0) / 2;           // (a clamped piece is never used: its rows are >= n)
        }
        const double2 *q2 = reinterpret_cast<const double2 *>(Q);
        const int64_t ld2 = ld / 2;
        int j = first;
        for (; j + U <= rows; j += U) {
            double2 x[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) x[u][v] = q2[(int64_t)(j + u) * ld2 + off[v]];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double cj = c[j + u];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    acc[v].x += cj * x[u][v].x;
                    acc[v].y += cj * x[u][v].y;
                }
            }
        }
        for (; j < rows; ++j) {
            const double cj = c[j];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double2 x = q2[(int64_t)j * ld2 + off[v]];
                acc[v].x += cj * x.x;
                acc[v].y += cj * x.y;
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int r = 2 * (threadIdx.x + v * kLz64Threads);
            const double a[2] = {acc[v].x, acc[v].y};
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (r0 + r + e < n) {
                    const double val = wv[r + e] - a[e];
                    wv[r + e] = val;
                    w[r0 + r + e] = val;
                    ss += val * val;
                }
        }
    } else {
        constexpr int JS = kLz64Threads / SPAN;             // 1 (SPAN 1024) or 4 (SPAN 256)
        constexpr int U = 8;
        const int r = threadIdx.x % SPAN, js = threadIdx.x / SPAN;
        const bool ok = r0 + r < n;
        const double *q = Q + (ok ? r0 + r : 0);
        double acc = 0.0;
        int j = first + js;
        for (; j + (U - 1) * JS < rows; j += U * JS) {
            double x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = q[(int64_t)(j + u * JS) * ld];
#pragma unroll
            for (int u = 0; u < U; ++u) acc += c[j + u * JS] * x[u];
        }
        for (; j < rows; j += JS) acc += c[j] * q[(int64_t)j * ld];
        if constexpr (JS > 1) {
            red[threadIdx.x] = acc;
            __syncthreads();
            acc = 0.0;
            if (js == 0) {
#pragma unroll
                for (int k = 0; k < JS; ++k) acc += red[k * SPAN + r];
            }
        }
        if (js == 0 && ok) {
            const double val = wv[r] - acc;
            wv[r] = val;
            w[r0 + r] = val;
            ss = val * val;
        }
    }
    return ss;
}

template <int SPAN>
__device__ __forceinline__ void lz64_stage(const double *__restrict__ w, int64_t r0, int64_t n, double *wv)
{
    for (int r = threadIdx.x; r < SPAN; r += kLz64Threads) wv[r] = r0 + r < n ? w[r0 + r] : 0.0;
    __syncthreads();
}

template <int SPAN>
__global__ __launch_bounds__(kLz64Threads) void lanczos64_project_kernel(const double *__restrict__ Q, int64_t ld,
                                                                         const double *__restrict__ w, int64_t n, int rows,
                                                                         double *__restrict__ partial)
{
    __shared__ double wv[SPAN];
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    lz64_stage<SPAN>(w, r0, n, wv);
    lz64_project<SPAN>(Q, ld, max(0, rows - 2), rows, r0, n, wv, partial + (size_t)blockIdx.x * kLz64MaxRows);
}

template <int SPAN>
__global__ __launch_bounds__(kLz64Threads) void lanczos64_subtract_project_kernel(const double *__restrict__ Q, int64_t ld,
                                                                                  double *__restrict__ w, int64_t n, int rows,
                                                                                  const double *__restrict__ partial_in, int groups,
                                                                                  double *__restrict__ partial_out,
                                                                                  double *__restrict__ c_out)
{
    __shared__ double wv[SPAN];
    __shared__ double red[kLz64Threads];
    __shared__ double c[kLz64MaxRows];
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    const int first = max(0, rows - 2);
    lz64_sum_groups(partial_in, groups, first, rows, red, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) c_out[0] = c[rows - 1];          // the first part of alpha_i
    lz64_stage<SPAN>(w, r0, n, wv);
    lz64_subtract<SPAN>(Q, ld, first, rows, r0, n, c, wv, red, w);
    __syncthreads();
    lz64_project<SPAN>(Q, ld, 0, rows, r0, n, wv, partial_out + (size_t)blockIdx.x * kLz64MaxRows);
}

template <int SPAN>
__global__ __launch_bounds__(kLz64Threads) void lanczos64_subtract_norm_kernel(const double *__restrict__ Q, int64_t ld,
                                                                               double *__restrict__ w, int64_t n, int rows,
                                                                               const double *__restrict__ partial_in, int groups,
                                                                               const double *__restrict__ c_first,
                                                                               double *__restrict__ alphas,
                                                                               double *__restrict__ sumsq)
{
    __shared__ double wv[SPAN];
    __shared__ double red[kLz64Threads];
    __shared__ double c[kLz64MaxRows];
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    lz64_sum_groups(partial_in, groups, 0, rows, red, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) alphas[rows - 1] = c_first[0] + c[rows - 1];
    lz64_stage<SPAN>(w, r0, n, wv);
    double ss = lz64_subtract<SPAN>(Q, ld, 0, rows, r0, n, c, wv, red, w);
    // sum of squares of the group: within the waves, then the waves in sequence
    const double ws = lz64_wave_sum(ss);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < kLz64Threads / 64; ++k) s += red[k];
        sumsq[blockIdx.x] = s;
    }
}

// beta = sqrt(sum over the groups of sumsq[g]), by the first wave of every workgroup: lane l takes groups l, l + 64, ... in
// order, then the lanes meet in a butterfly (the same tree in every workgroup and every call)
template <int SPAN>
__global__ __launch_bounds__(kLz64Threads) void lanczos64_scale_kernel(const double *__restrict__ w, int64_t n,
                                                                       const double *__restrict__ sumsq, int groups,
                                                                       double *__restrict__ qnext, double *__restrict__ betas, int i)
{
    __shared__ double div_s;
    if (threadIdx.x < 64) {
        double s = 0.0;
        for (int g = threadIdx.x; g < groups; g += 64) s += sumsq[g];
        s = lz64_wave_sum(s);
        if (threadIdx.x == 0) {
            const double beta = sqrt(s);
            div_s = fmax(beta, 1e-300);
            if (blockIdx.x == 0) betas[i] = beta;
        }
    }
    __syncthreads();
    const double div = div_s;
    const int64_t r0 = (int64_t)blockIdx.x * SPAN;
    for (int k = threadIdx.x; k < SPAN; k += kLz64Threads)
        if (r0 + k < n) qnext[r0 + k] = w[r0 + k] / div;
}

template <int SPAN>
static void lanczos64_launch(double *Q, int64_t ld, double *w, int64_t n, int i, double *alphas, double *betas, double *work,
                             int groups, hipStream_t s)
{
    double *p0 = work, *p1 = work + (size_t)kLz64MaxGroups * kLz64MaxRows, *c0 = p1 + (size_t)kLz64MaxGroups * kLz64MaxRows,
           *sumsq = c0 + kLz64MaxRows;
    const int rows = i + 1;
    lanczos64_project_kernel<SPAN><<<groups, kLz64Threads, 0, s>>>(Q, ld, w, n, rows, p0);
    lanczos64_subtract_project_kernel<SPAN><<<groups, kLz64Threads, 0, s>>>(Q, ld, w, n, rows, p0, groups, p1, c0);
    lanczos64_subtract_norm_kernel<SPAN><<<groups, kLz64Threads, 0, s>>>(Q, ld, w, n, rows, p1, groups, c0, alphas, sumsq);
    lanczos64_scale_kernel<SPAN><<<groups, kLz64Threads, 0, s>>>(w, n, sumsq, groups, Q + (size_t)(i + 1) * ld, betas, i);
}

} // namespace plx

using namespace plx;

extern "C" int64_t plx_lanczos_work_doubles(int64_t n)
{
    if (n < 1 || lanczos64_shape(n).groups > kLz64MaxGroups) return -1;
    return 2 * (int64_t)kLz64MaxGroups * kLz64MaxRows + kLz64MaxRows + kLz64MaxGroups;
}

extern "C" int plx_lanczos_shape_f64(int64_t n, int *span, int *groups)
{
    if (plx_lanczos_work_doubles(n) < 0) {
        set_error("plx_lanczos_shape_f64: n = %lld outside 1..%lld", (long long)n, (long long)kLz64MaxGroups * kLz64MaxSpan);
        return PLX_ERR_INVALID;
    }
    const Lz64Shape sh = lanczos64_shape(n);
    if (span) *span = sh.span;
    if (groups) *groups = sh.groups;
    return PLX_OK;
}

extern "C" int plx_lanczos_step_f64(double *d_q, int64_t ld, double *d_w, int64_t n, int i, double *d_alphas, double *d_betas,
                                    double *d_work, void *stream)
{
    const char *who = "plx_lanczos_step_f64";
    if (!d_q || !d_w || !d_alphas || !d_betas || !d_work) {
        set_error("%s: NULL argument", who);
        return PLX_ERR_INVALID;
    }
    const uintptr_t bits = (uintptr_t)d_q | (uintptr_t)d_w | (uintptr_t)d_alphas | (uintptr_t)d_betas | (uintptr_t)d_work;
    if ((bits & 7) != 0) {
        set_error("%s: buffers of doubles must be 8-byte aligned", who);
        return PLX_ERR_INVALID;
    }
    if (n < 1 || ld < n || i < 0 || i + 1 > kLz64MaxRows) {
        set_error("%s: n = %lld, ld = %lld, step %d (n >= 1, ld >= n, at most %d basis vectors)", who, (long long)n, (long long)ld, i,
                  kLz64MaxRows);
        return PLX_ERR_INVALID;
    }
    if (ld % 2 != 0 || ((uintptr_t)d_q & 15) != 0) {
        set_error("%s: the basis must be 16-byte aligned with ld a multiple of 2 (ld = %lld)", who, (long long)ld);
        return PLX_ERR_INVALID;
    }
    const Lz64Shape sh = lanczos64_shape(n);
    if (sh.groups > kLz64MaxGroups) {
        set_error("%s: n = %lld is more than %lld rows", who, (long long)n, (long long)kLz64MaxGroups * kLz64MaxSpan);
        return PLX_ERR_INVALID;
    }
    // w is read and written while rows 0..i of the basis are read and row i + 1 is written: no part of it inside them
    if (d_w < d_q + (size_t)(i + 2) * ld && d_w + n > d_q) {
        set_error("%s: d_w overlaps rows 0..%d of the basis", who, i + 1);
        return PLX_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (sh.span) {
    case 256: lanczos64_launch<256>(d_q, ld, d_w, n, i, d_alphas, d_betas, d_work, sh.groups, s); break;
    case 1024: lanczos64_launch<1024>(d_q, ld, d_w, n, i, d_alphas, d_betas, d_work, sh.groups, s); break;
    default: lanczos64_launch<kLz64MaxSpan>(d_q, ld, d_w, n, i, d_alphas, d_betas, d_work, sh.groups, s); break;
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}
