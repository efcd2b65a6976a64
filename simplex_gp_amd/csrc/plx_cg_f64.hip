// plx_cg_f64.hip -- the float64 conjugate-gradient solve next to the float64 product (include/plx.h: plx_coldot_f64,
// plx_cg_step_update_f64, plx_cg_step_direction_f64, plx_apply_affine_f64; the entry point of the last one and its argument
// checks are in plx_api.hip, beside plx_apply_f64).
//
// The three vector calls are plx_cg_kernels.h with T = double: this file holds the float64 kernels, the entry points (n >= 1,
// every buffer 8-byte aligned: cg_rules_f64) and the two launchers the preconditioned iteration shares (plx_internal.h): its
// <R, Z> is summed by coldot_final, its direction step is cg_step_direction, and plx_pcg_f64.hip checks its pointers with
// cg_check under the same rules.
//
// The affine slice is plx_f64.hip's slice (the same three shapes, the same gates, the sums formed from the same pieces
// of plx_kernels.h in the same order, ONE division by 1 + 2^-d) with the tail out = fma(a, y, b x) fused: the slice already
// holds the point's caller row from the permutation and reads src there.  With (a, b) = (1, 0) that is y + 0 = y: the
// values of plx_apply_f64.  The v1 and chunk shapes can also leave <src, out> per column as one partial row per workgroup
// (tree over the workgroup's points in LDS, fixed order), added up by the final stage of plx_coldot_f64.

#include "plx_cg_kernels.h"
#include "plx_kernels.h"

namespace plx {

PLX_CG_INSTANTIATE(double)

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

}  // namespace plx

using namespace plx;

extern "C" int64_t plx_coldot_work_doubles(int vd) { return (vd >= 1 && vd <= kBlock) ? (int64_t)kDotBlocks * vd : -1; }

extern "C" int plx_coldot_f64(const double *d_a, const double *d_b, int64_t n, int vd, double *d_out, double *d_work,
                              void *stream)
{
    return cg_coldot(cg_rules_f64("plx_coldot_f64"), d_a, d_b, n, vd, d_out, d_work, (hipStream_t)stream);
}

extern "C" int plx_cg_step_update_f64(double *d_x, double *d_r, const double *d_p, const double *d_ap, const double *d_rs,
                                      const double *d_pap, const double *d_active, int64_t n, int vd, double *d_rs_new,
                                      double *d_alpha, double *d_work, void *stream)
{
    return cg_step_update(cg_rules_f64("plx_cg_step_update_f64"), d_x, d_r, d_p, d_ap, d_rs, d_pap, d_active, n, vd, d_rs_new,
                          d_alpha, d_work, (hipStream_t)stream);
}

extern "C" int plx_cg_step_direction_f64(double *d_p, const double *d_r, const double *d_rs_new, const double *d_rs,
                                         const double *d_active, const double *d_b_norm, double tol, int64_t n, int vd,
                                         double *d_beta, double *d_active_out, void *stream)
{
    return cg_step_direction(cg_rules_f64("plx_cg_step_direction_f64"), d_p, d_r, d_rs_new, d_rs, d_rs_new, d_active, d_b_norm,
                             tol, n, vd, d_beta, d_active_out, (hipStream_t)stream);
}
