// plx_cg_f64.hip -- the float64 conjugate-gradient solve next to the float64 product (include/plx.h: plx_coldot_f64,
// plx_cg_step_update_f64, plx_cg_step_direction_f64, plx_apply_affine_f64; the entry point of the last one and its argument
// checks are in plx_api.hip, beside plx_apply_f64).
//
// The three vector calls are plx_linalg.hip's plx_coldot / plx_cg_step_update / plx_cg_step_direction with every array in
// double and the guard max(x, 1e-300) (a right-hand side scaled by 1e-20 has pAp near 1e-40: the fp32 guard 1e-30 would
// turn its alpha into garbage).  Thread mapping as there: (row lane, column lane), column fastest, vd lanes per row, so
// consecutive threads read consecutive doubles -- a 64-lane wave covers 512 consecutive bytes whatever vd is, and a
// power-of-two lane count per row would idle 5 of 16 lanes at vd = 11.  Per-workgroup partial sums through LDS in a fixed
// order, then one workgroup per column adds the partial rows in a fixed order: no atomics, bitwise reproducible.
// The preconditioned iteration shares this file's steps (plx_internal.h): its <R, Z> is summed by coldot_final_f64, its
// direction step is step_direction_f64, and plx_pcg_f64.hip checks its pointers with check_cg64.
//
// The affine slice is plx_f64.hip's slice (the same three shapes, the same gates, the sums formed from the same pieces
// of plx_kernels.h in the same order, ONE division by 1 + 2^-d) with the tail out = fma(a, y, b x) fused: the slice already
// holds the point's caller row from the permutation and reads src there.  With (a, b) = (1, 0) that is y + 0 = y: the
// values of plx_apply_f64.  The v1 and chunk shapes can also leave <src, out> per column as one partial row per workgroup
// (tree over the workgroup's points in LDS, fixed order), added up by the final stage of plx_coldot_f64.

#include "plx_kernels.h"

#include <math.h>

namespace plx {

constexpr int kDot64Blocks = 1024;
constexpr int kFinal64Block = 1024;
constexpr double kTiny64 = 1e-300;

// ---- column dots and the two CG steps -----------------------------------------------------------------------------------
// fixed-order sum over the row lanes of each column: red[k * cw + c], k = 0 .. rows_per_step - 1
__device__ __forceinline__ void cg64_store_partial(const double *red, int c, int rl, int cw, int vd, int rows_per_step,
                                                   double *__restrict__ partial)
{
    if (rl == 0 && c < vd) {
        double s = 0.0;
        for (int k = 0; k < rows_per_step; ++k) s += red[k * cw + c];
        partial[(size_t)blockIdx.x * vd + c] = s;
    }
}

__global__ __launch_bounds__(kBlock) void coldot64_partial_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                                  int64_t n, int vd, int cw, double *__restrict__ partial)
{
    __shared__ double red[kBlock];
    const int c = threadIdx.x % cw;
    const int rl = threadIdx.x / cw;
    const int rows_per_step = kBlock / cw;
    const int64_t rows_per_block = (n + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + rows_per_block, n);
    double acc = 0.0;
    if (rl < rows_per_step)                              // (the last kBlock % vd threads have no row lane)
        for (int64_t r = r0 + rl; r < r1; r += rows_per_step) acc += a[r * vd + c] * b[r * vd + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    cg64_store_partial(red, c, rl, cw, vd, rows_per_step, partial);
}

// One workgroup per column over `nrows` partial rows of `stride` doubles: thread-strided sums (four loads in flight), then
// a tree.
__global__ __launch_bounds__(kFinal64Block) void coldot64_final_kernel(const double *__restrict__ partial, int nrows,
                                                                       int stride, double *__restrict__ out)
{
    __shared__ double red[kFinal64Block];
    const int c = blockIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int k = threadIdx.x;
    for (; k + 3 * kFinal64Block < nrows; k += 4 * kFinal64Block) {
        const double p0 = partial[(size_t)k * stride + c], p1 = partial[(size_t)(k + kFinal64Block) * stride + c];
        const double p2 = partial[(size_t)(k + 2 * kFinal64Block) * stride + c];
        const double p3 = partial[(size_t)(k + 3 * kFinal64Block) * stride + c];
        a0 += p0; a1 += p1; a2 += p2; a3 += p3;
    }
    for (; k < nrows; k += kFinal64Block) a0 += partial[(size_t)k * stride + c];
    red[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    for (int s = kFinal64Block / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = red[0];
}

//   step_update:     alpha = active ? rs / max(pAp, tiny) : 0;  X += alpha P;  R -= alpha AP;  partial |R|^2
__global__ __launch_bounds__(kBlock) void cg64_step_update_kernel(double *__restrict__ X, double *__restrict__ R,
                                                                  const double *__restrict__ P, const double *__restrict__ AP,
                                                                  const double *__restrict__ rs, const double *__restrict__ pAp,
                                                                  const double *__restrict__ active, int64_t n, int vd, int cw,
                                                                  double *__restrict__ partial, double *__restrict__ alpha_out)
{
    __shared__ double red[kBlock];
    const int c = threadIdx.x % cw;
    const int rl = threadIdx.x / cw;
    const int rows_per_step = kBlock / cw;
    const int64_t rows_per_block = (n + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + rows_per_block, n);
    double acc = 0.0;
    if (rl < rows_per_step) {
        const double a = active[c] > 0.0 ? rs[c] / fmax(pAp[c], kTiny64) : 0.0;
        if (blockIdx.x == 0 && rl == 0) alpha_out[c] = a;
        for (int64_t r = r0 + rl; r < r1; r += rows_per_step) {
            const int64_t i = r * vd + c;
            X[i] += P[i] * a;
            const double res = R[i] - AP[i] * a;
            R[i] = res;
            acc += res * res;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    cg64_store_partial(red, c, rl, cw, vd, rows_per_step, partial);
}

// The direction step of a plain and of a preconditioned iteration: P = src + beta P, beta = active ? num / max(den, tiny) : 0,
// active' = active and sqrt(rr) / b_norm > tol.  CG: src = R, num = rr = |R'|^2, den = |R|^2 (num and rr are then one
// read-only pointer); PCG: src = Z, num = <R', Z'>, den = <R, Z>, rr = the true |R'|^2.
__device__ __forceinline__ double direction64_beta(const double *num, const double *den, const double *active, int c)
{
    return active[c] > 0.0 ? num[c] / fmax(den[c], kTiny64) : 0.0;
}

__device__ __forceinline__ void direction64_scalars(const double *num, const double *den, const double *rr,
                                                    const double *active, const double *b_norm, double tol, int vd,
                                                    double *beta_out, double *active_out)
{
    if (blockIdx.x == 0 && (int)threadIdx.x < vd) {
        const int c = threadIdx.x;
        beta_out[c] = direction64_beta(num, den, active, c);
        active_out[c] = (active[c] > 0.0 && sqrt(rr[c]) / b_norm[c] > tol) ? 1.0 : 0.0;
    }
}

// beta per column once per workgroup; the column of element i = blockIdx * kBlock + tid from 32-bit residues
__global__ __launch_bounds__(kBlock) void step_direction64_kernel(double *__restrict__ P, const double *__restrict__ src,
                                                                  const double *__restrict__ num,
                                                                  const double *__restrict__ den,
                                                                  const double *__restrict__ rr,
                                                                  const double *__restrict__ active,
                                                                  const double *__restrict__ b_norm, double tol,
                                                                  int64_t total, int vd, double *__restrict__ beta_out,
                                                                  double *__restrict__ active_out)
{
    __shared__ double sbeta[kBlock];
    if ((int)threadIdx.x < vd) sbeta[threadIdx.x] = direction64_beta(num, den, active, threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < total) {
        const uint32_t uvd = (uint32_t)vd;
        const uint32_t bm = ((blockIdx.x % uvd) * ((uint32_t)kBlock % uvd)) % uvd;      // wave-uniform
        const uint32_t c = (bm + threadIdx.x) % uvd;
        P[i] = src[i] + P[i] * sbeta[c];
    }
    direction64_scalars(num, den, rr, active, b_norm, tol, vd, beta_out, active_out);
}

// the same two elements per thread (16-byte loads / stores; total even, P and src 16-byte aligned)
__global__ __launch_bounds__(kBlock) void step_direction64_pair_kernel(double2 *__restrict__ P, const double2 *__restrict__ src,
                                                                       const double *__restrict__ num,
                                                                       const double *__restrict__ den,
                                                                       const double *__restrict__ rr,
                                                                       const double *__restrict__ active,
                                                                       const double *__restrict__ b_norm, double tol,
                                                                       int64_t pairs, int vd, double *__restrict__ beta_out,
                                                                       double *__restrict__ active_out)
{
    __shared__ double sbeta[kBlock];
    if ((int)threadIdx.x < vd) sbeta[threadIdx.x] = direction64_beta(num, den, active, threadIdx.x);
    __syncthreads();
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q < pairs) {
        const uint32_t uvd = (uint32_t)vd;
        // column of element 2 q = 2 (blockIdx kBlock + tid) mod vd, from 32-bit residues
        const uint32_t bm = ((blockIdx.x % uvd) * ((2u * (uint32_t)kBlock) % uvd)) % uvd;      // wave-uniform
        uint32_t c = (bm + 2u * threadIdx.x) % uvd;
        const double2 r = src[q];
        double2 p = P[q];
        p.x = r.x + p.x * sbeta[c]; c = c + 1 == uvd ? 0 : c + 1;
        p.y = r.y + p.y * sbeta[c];
        P[q] = p;
    }
    direction64_scalars(num, den, rr, active, b_norm, tol, vd, beta_out, active_out);
}

// ---- the slice with the affine tail ----------------------------------------------------------------------------------------
// the workgroup's contributions to <src, out>, one V per thread (zero where the thread holds no element): a tree over the
// groups of G = 1 << shift lanes leaves the sums of lane ch's column(s) in red[ch]
template <class V>
__device__ __forceinline__ void f64_dot_tree(V *red, V mine, int shift)
{
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int s = kBlock / 2; s >= (1 << shift); s >>= 1) {
        if ((int)threadIdx.x < s) {
            if constexpr (std::is_same<V, double>::value) red[threadIdx.x] += red[threadIdx.x + s];
            else { red[threadIdx.x].x += red[threadIdx.x + s].x; red[threadIdx.x].y += red[threadIdx.x + s].y; }
        }
        __syncthreads();
    }
}

// D1 > 0: d + 1 compiled in (all index / weight loads, then all gathers, then the ordered sum); 0: the run-time form.
// partial != NULL: one double per workgroup, the sum of src * out over its points.
template <int D1>
__global__ __launch_bounds__(kBlock) void f64_affine_v1_kernel(const uint32_t *__restrict__ perm, const int *__restrict__ evid,
                                                               const float *__restrict__ ew, int n, int d1,
                                                               const double *__restrict__ values, double denom,
                                                               const double *__restrict__ src, const double *__restrict__ ss,
                                                               double *__restrict__ out, double *__restrict__ partial)
{
    __shared__ double red[kBlock];
    const int p = blockIdx.x * kBlock + threadIdx.x;
    double mine = 0.0;
    if (p < n) {
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
        const double y = acc / denom;
        const size_t row = perm[p];
        const double x = src[row];
        const double o = fma(ss[0], y, ss[1] * x);
        out[row] = o;
        mine = x * o;
    }
    if (partial) {                                       // (uniform over the launch)
        f64_dot_tree(red, mine, 0);
        if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
    }
}

__device__ __forceinline__ double2 f64_affine_tail(double2 y, double2 x, const double *__restrict__ ss)
{
    const double a = ss[0], b = ss[1];
    return make_double2(fma(a, y.x, b * x.x), fma(a, y.y, b * x.y));
}

// partial != NULL: one row of 2 nch doubles per workgroup (the padding column of an odd vd gets 0: its src reads as 0)
template <bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void f64_affine_chunk_kernel(const uint32_t *__restrict__ perm,
                                                                  const int *__restrict__ evid, const float *__restrict__ ew,
                                                                  int n, int d1, const double2 *__restrict__ values, int vd,
                                                                  int nch, int shift, double denom,
                                                                  const double *__restrict__ src, const double *__restrict__ ss,
                                                                  double *__restrict__ out, double *__restrict__ partial)
{
    __shared__ double2 red[kBlock];
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t p64 = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    double2 mine = VecOps<double2>::zero();
    if (p64 < n && ch < nch) {
        const int p = (int)p64;
        double2 acc;
        if constexpr (D1 > 0) {
            int v[D1];
            double2 g[D1];
#pragma unroll
            for (int r = 0; r < D1; ++r) v[r] = evid[(size_t)r * n + p];
#pragma unroll
            for (int r = 0; r < D1; ++r) g[r] = values[(size_t)v[r] * nch + ch];
            acc = VecOps<double2>::zero();
#pragma unroll
            for (int r = 0; r < D1; ++r) VecOps<double2>::fma(acc, (double)ew[(size_t)r * n + p], g[r]);
            acc = make_double2(acc.x / denom, acc.y / denom);
        } else {
            acc = f64_point_sum(evid, ew, n, p, d1, values, nch, ch, denom);
        }
        const size_t row = (size_t)perm[p];
        const double2 x = f64_load_chunk<VEC>(src, row, vd, ch);
        const double2 o = f64_affine_tail(acc, x, ss);
        f64_store_chunk<VEC>(out, row, vd, ch, o);
        mine = make_double2(x.x * o.x, x.y * o.y);
    }
    if (partial) {                                       // (uniform over the launch)
        f64_dot_tree(red, mine, shift);
        if ((int)threadIdx.x < nch) {                    // nch <= 1 << shift: red[ch] holds chunk ch's two column sums
            double *o = partial + ((size_t)blockIdx.x * nch + threadIdx.x) * 2;
            o[0] = red[threadIdx.x].x;
            o[1] = red[threadIdx.x].y;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void f64_affine_wide_kernel(const uint32_t *__restrict__ perm,
                                                                 const int *__restrict__ evid, const float *__restrict__ ew,
                                                                 int n, int d1, const double2 *__restrict__ values, int vd,
                                                                 int nch, double denom, const double *__restrict__ src,
                                                                 const double *__restrict__ ss, double *__restrict__ out)
{
    const int64_t p64 = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (p64 >= n) return;
    const int p = (int)p64;
    const size_t row = (size_t)perm[p];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64) {
        const double2 y = f64_point_sum(evid, ew, n, p, d1, values, nch, ch, denom);
        f64_store_chunk<VEC>(out, row, vd, ch, f64_affine_tail(y, f64_load_chunk<VEC>(src, row, vd, ch), ss));
    }
}

// ---- launch side -----------------------------------------------------------------------------------------------------
// workgroups of the v1 / chunk affine slice = partial rows of its dot; 0 where the dot is not served (the wide shape)
int affine_f64_dot_rows(const plx_lattice *L, int vd)
{
    if (vd == 1) return ceil_div(L->n, kBlock);
    const int nch = values_stride_f64(vd) / 2;
    if (nch > kChunkGroupMax) return 0;
    return ceil_div((int64_t)L->n << chunk_group_shift(nch), kBlock);
}

template <bool VEC>
static void launch_affine_chunk_f64(plx_lattice *L, const double2 *v2, int vd, int nch, double denom, const double *d_src,
                                    const double *d_ss, double *d_out, double *d_partial, hipStream_t stream)
{
    const int n = (int)L->n, d1 = L->d + 1;
    const int shift = chunk_group_shift(nch);
    const int grid = ceil_div((int64_t)n << shift, kBlock);
    const uint32_t *perm = L->perm.as<uint32_t>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    dispatch_d1(d1, [&](auto D1) {
        f64_affine_chunk_kernel<VEC, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, v2, vd, nch, shift,
                                                                                       denom, d_src, d_ss, d_out, d_partial);
    });
}

int coldot_final_f64(const double *d_partial, int nrows, int stride, int vd, double *d_out, hipStream_t stream)
{
    coldot64_final_kernel<<<vd, kFinal64Block, 0, stream>>>(d_partial, nrows, stride, d_out);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

// d_partial (optional; v1 and chunk shapes only): affine_f64_dot_rows(L, vd) rows of values_stride_f64(vd) doubles
int slice_affine_f64_impl(plx_lattice *L, const double *d_values, int vd, const double *d_src, const double *d_ss,
                          double *d_out, double *d_partial, hipStream_t stream)
{
    const int n = (int)L->n, d1 = L->d + 1, nch = values_stride_f64(vd) / 2;
    const double denom = 1.0 + ldexp(1.0, -L->d);
    const uint32_t *perm = L->perm.as<uint32_t>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    const bool vec = f64_vec_ok(d_out, vd) && f64_vec_ok(d_src, vd);
    const double2 *v2 = reinterpret_cast<const double2 *>(d_values);
    if (vd == 1) {
        L->kn_f64_slice = "f64_affine_v1_kernel";
        const int grid = ceil_div(n, kBlock);
        dispatch_d1(d1, [&](auto D1) {
            f64_affine_v1_kernel<decltype(D1)::value><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, d_values, denom,
                                                                                   d_src, d_ss, d_out, d_partial);
        });
    } else if (nch <= kChunkGroupMax) {
        L->kn_f64_slice = "f64_affine_chunk_kernel";
        if (vec) launch_affine_chunk_f64<true>(L, v2, vd, nch, denom, d_src, d_ss, d_out, d_partial, stream);
        else launch_affine_chunk_f64<false>(L, v2, vd, nch, denom, d_src, d_ss, d_out, d_partial, stream);
    } else {
        L->kn_f64_slice = "f64_affine_wide_kernel";
        const int grid = ceil_div(n, kBlock / 64);
        if (vec) f64_affine_wide_kernel<true><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, v2, vd, nch, denom, d_src, d_ss, d_out);
        else f64_affine_wide_kernel<false><<<grid, kBlock, 0, stream>>>(perm, evid, ew, n, d1, v2, vd, nch, denom, d_src, d_ss, d_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

// Everything a vector call checks before any launch.  ptrs: every pointer argument of the call.
int check_cg64(const char *who, std::initializer_list<const void *> ptrs, int64_t n, int vd)
{
    uintptr_t bits = 0;
    for (const void *q : ptrs) {
        if (!q) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
        bits |= (uintptr_t)q;
    }
    if (vd < 1 || vd > kBlock) { set_error("%s: vd = %d outside 1..%d", who, vd, kBlock); return PLX_ERR_INVALID; }
    if (n < 1) { set_error("%s: n = %lld must be positive", who, (long long)n); return PLX_ERR_INVALID; }
    if ((bits & 7) != 0) { set_error("%s: buffers of doubles must be 8-byte aligned", who); return PLX_ERR_INVALID; }
    return PLX_OK;
}

int step_direction_f64(const char *who, double *d_p, const double *d_src, const double *d_num, const double *d_den,
                       const double *d_rr, const double *d_active, const double *d_b_norm, double tol, int64_t n, int vd,
                       double *d_beta, double *d_active_out, hipStream_t s)
{
    PLX_TRY(check_cg64(who, {d_p, d_src, d_num, d_den, d_rr, d_active, d_b_norm, d_beta, d_active_out}, n, vd));
    if (d_active == d_active_out) { set_error("%s: active and active_out must be different buffers", who); return PLX_ERR_INVALID; }
    const int64_t total = n * vd;
    if ((total & 1) == 0 && ((reinterpret_cast<uintptr_t>(d_p) | reinterpret_cast<uintptr_t>(d_src)) & 15) == 0) {
        const int64_t pairs = total / 2;
        step_direction64_pair_kernel<<<ceil_div(pairs, kBlock), kBlock, 0, s>>>(
            reinterpret_cast<double2 *>(d_p), reinterpret_cast<const double2 *>(d_src), d_num, d_den, d_rr, d_active, d_b_norm,
            tol, pairs, vd, d_beta, d_active_out);
    } else {
        step_direction64_kernel<<<ceil_div(total, kBlock), kBlock, 0, s>>>(d_p, d_src, d_num, d_den, d_rr, d_active, d_b_norm, tol,
                                                                          total, vd, d_beta, d_active_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx

using namespace plx;

extern "C" int64_t plx_coldot_work_doubles(int vd) { return (vd >= 1 && vd <= kBlock) ? (int64_t)kDot64Blocks * vd : -1; }

extern "C" int plx_coldot_f64(const double *d_a, const double *d_b, int64_t n, int vd, double *d_out, double *d_work,
                              void *stream)
{
    PLX_TRY(check_cg64("plx_coldot_f64", {d_a, d_b, d_out, d_work}, n, vd));
    hipStream_t s = (hipStream_t)stream;
    coldot64_partial_kernel<<<kDot64Blocks, kBlock, 0, s>>>(d_a, d_b, n, vd, vd, d_work);      // cw = vd lanes per row
    coldot64_final_kernel<<<vd, kFinal64Block, 0, s>>>(d_work, kDot64Blocks, vd, d_out);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

extern "C" int plx_cg_step_update_f64(double *d_x, double *d_r, const double *d_p, const double *d_ap, const double *d_rs,
                                      const double *d_pap, const double *d_active, int64_t n, int vd, double *d_rs_new,
                                      double *d_alpha, double *d_work, void *stream)
{
    PLX_TRY(check_cg64("plx_cg_step_update_f64", {d_x, d_r, d_p, d_ap, d_rs, d_pap, d_active, d_rs_new, d_alpha, d_work}, n, vd));
    hipStream_t s = (hipStream_t)stream;
    cg64_step_update_kernel<<<kDot64Blocks, kBlock, 0, s>>>(d_x, d_r, d_p, d_ap, d_rs, d_pap, d_active, n, vd, vd, d_work, d_alpha);
    coldot64_final_kernel<<<vd, kFinal64Block, 0, s>>>(d_work, kDot64Blocks, vd, d_rs_new);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

extern "C" int plx_cg_step_direction_f64(double *d_p, const double *d_r, const double *d_rs_new, const double *d_rs,
                                         const double *d_active, const double *d_b_norm, double tol, int64_t n, int vd,
                                         double *d_beta, double *d_active_out, void *stream)
{
    return step_direction_f64("plx_cg_step_direction_f64", d_p, d_r, d_rs_new, d_rs, d_rs_new, d_active, d_b_norm, tol, n, vd,
                              d_beta, d_active_out, (hipStream_t)stream);
}
