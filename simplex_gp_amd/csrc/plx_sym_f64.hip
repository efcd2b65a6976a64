// plx_sym_f64.hip -- the transposed and the symmetrised float64 blur on a built lattice: plx_blur_t_f64 / plx_blur_sym_f64
// and the products around them (include/plx.h; the entry points and their argument checks are in plx_api.hip).
//
// The operator K = S B_d ... B_0 S^T / (1 + 2^-d) is not symmetric: the d + 1 axis blurs do not commute.  On a plain
// build the neighbour table is symmetric (u is the +j neighbour of v exactly when v is the -j neighbour of u), so the
// transpose of one axis blur is the same axis with the taps mirrored, c'[i] = c[2 r - i], and
//   K^T = S B'_0 ... B'_d S^T / (1 + 2^-d):  the axes in reverse order, mirrored taps -- host code around the kernels
//         of plx_f64.hip (blur_axis_f64), nothing new on the device;
//   K_s = (K + K^T) / 2 = S  (B_fwd + B_rev) / 2  S^T / (1 + 2^-d):  one splat, two blur chains, one slice.
//
// f64_blur_dual_kernel advances both chains in one launch: launch k of d + 1 takes the forward chain F through axis k
// and the reverse chain R through axis d - k.  One thread per (vertex, chunk) as in f64_blur_item, all 4 r neighbour ids
// in flight, then all 4 r gathers and the two centres, then each chain's sum in f64_blur_item's slot order with its
// fmas -- so F and R hold, launch by launch, the bits plx_blur_f64 and plx_blur_t_f64 hold after as many axes.
//   FIRST  both chains read the one splat plane (no copy);
//   LAST   the launch stores the single plane 0.5 (F + R): one rounded sum, the halving exact;
//   k == d - k (the middle launch of an even d): both chains gather through the same ids, loaded once.
// Planes: F and R are SEPARATE planes of m rows, not interleaved rows.  A chain's gathers follow the lattice order along
// one axis, and tile_index keeps every XCD inside one eighth of the plane it gathers from; rows interleaved [F | R] would
// double the stride between the rows one chain gathers -- half of every fetched line (vd = 1: 8 useful bytes in 16) the
// other chain's, which gathers along another axis -- and halve what an XCD's L2 holds of either.  Four planes in all
// (d_values + three of work): a launch reads one pair and writes the other, so no thread stores where another still
// gathers; the last launch writes a plane of the pair it does not read.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, bitwise reproducible.

#include "plx_kernels.h"

#include <utility>

namespace plx {

// One chain's sum over one axis: f64_blur_item's, from ids and gathers already in registers.
template <class V, int ORDER>
__device__ __forceinline__ V f64_dual_sum(const int (&id)[2 * ORDER + 1], const V (&g)[2 * ORDER + 1], V centre, const double *c)
{
    using O = VecOps<V>;
    V acc = O::zero();
#pragma unroll
    for (int s = 0; s < ORDER; ++s)
        if (id[s] >= 0) O::fma(acc, c[s], g[s]);
    O::fma(acc, c[ORDER], centre);
#pragma unroll
    for (int s = 0; s < ORDER; ++s)
        if (id[ORDER + s] >= 0) O::fma(acc, c[ORDER + 1 + s], g[ORDER + s]);
    return acc;
}

// ... and its run-time form (ORDER = -1): f64_blur_item's loop
template <class V>
__device__ __forceinline__ V f64_dual_sum_rt(const V *__restrict__ old, const int *__restrict__ nbr, int64_t mstride,
                                             uint32_t i, uint32_t ch, uint32_t item, int rowlen, int order, const double *c)
{
    using O = VecOps<V>;
    V acc = O::zero();
    for (int s = 0; s < order; ++s) {
        const int nb = nbr[s * mstride + i];
        if (nb >= 0) O::fma(acc, c[s], old[(size_t)nb * rowlen + ch]);
    }
    O::fma(acc, c[order], old[item]);
    for (int s = 0; s < order; ++s) {
        const int nb = nbr[(order + s) * mstride + i];
        if (nb >= 0) O::fma(acc, c[order + 1 + s], old[(size_t)nb * rowlen + ch]);
    }
    return acc;
}

// 0.5 (f + r): the sum rounded once on its own (never contracted into the fma that formed r), the halving exact
__device__ __forceinline__ double f64_half_sum(double f, double r)
{
#pragma clang fp contract(off)
    const double s = f + r;
    return 0.5 * s;
}
__device__ __forceinline__ double f64_mean(double f, double r) { return f64_half_sum(f, r); }
__device__ __forceinline__ double2 f64_mean(double2 f, double2 r) { return make_double2(f64_half_sum(f.x, r.x), f64_half_sum(f.y, r.y)); }

// V = double (vd = 1, rowlen 1) or double2 (rowlen chunks per vertex).  ORDER >= 0: compiled in; -1: order_rt.
// fin / rin: the planes the two chains read (FIRST: rin is not read, both read fin); fout / rout: the planes they write
// (LAST: fout receives 0.5 (F + R), rout is not written).  nbr_f / nbr_r: the neighbour tables of axis k and axis d - k.
template <class V, int ORDER, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBlock) void f64_blur_dual_kernel(const V *fin, const V *rin, V *fout, V *rout,
                                                               const int *__restrict__ nbr_f, const int *__restrict__ nbr_r,
                                                               int m, int64_t mstride, int rowlen, int order_rt, TapArgs64 taps_f,
                                                               TapArgs64 taps_r, int ntiles)
{
    const int tile = tile_index(ntiles);
    if (tile < 0) return;
    const uint32_t item = (uint32_t)tile * kBlock + threadIdx.x;      // (the entry point checks m * rowlen < 2^31)
    if (item >= (uint32_t)m * (uint32_t)rowlen) return;
    const uint32_t i = item / (uint32_t)rowlen, ch = item - i * (uint32_t)rowlen;
    const V *rsrc = FIRST ? fin : rin;
    const bool shared = nbr_f == nbr_r;       // the middle launch of an even d: one axis serves both chains
    V f, r;
    if constexpr (ORDER >= 0) {
        int idf[2 * ORDER + 1], idr[2 * ORDER + 1];
        V gf[2 * ORDER + 1], gr[2 * ORDER + 1];
#pragma unroll
        for (int s = 0; s < 2 * ORDER; ++s) idf[s] = nbr_f[s * mstride + i];
        if (shared) {
#pragma unroll
            for (int s = 0; s < 2 * ORDER; ++s) idr[s] = idf[s];
        } else {
#pragma unroll
            for (int s = 0; s < 2 * ORDER; ++s) idr[s] = nbr_r[s * mstride + i];
        }
#pragma unroll
        for (int s = 0; s < 2 * ORDER; ++s) gf[s] = fin[idf[s] >= 0 ? (size_t)idf[s] * rowlen + ch : (size_t)item];
#pragma unroll
        for (int s = 0; s < 2 * ORDER; ++s) gr[s] = rsrc[idr[s] >= 0 ? (size_t)idr[s] * rowlen + ch : (size_t)item];
        const V cf = fin[item];
        const V cr = FIRST ? cf : rsrc[item];
        f = f64_dual_sum<V, ORDER>(idf, gf, cf, taps_f.c);
        r = f64_dual_sum<V, ORDER>(idr, gr, cr, taps_r.c);
    } else {
        f = f64_dual_sum_rt<V>(fin, nbr_f, mstride, i, ch, item, rowlen, order_rt, taps_f.c);
        r = f64_dual_sum_rt<V>(rsrc, nbr_r, mstride, i, ch, item, rowlen, order_rt, taps_r.c);
    }
    if constexpr (LAST) {
        fout[item] = f64_mean(f, r);
    } else {
        fout[item] = f;
        rout[item] = r;
    }
}

// ---- launch side ---------------------------------------------------------------------------------------------------
static TapArgs64 taps_f64(const plx_lattice *L, bool mirrored)
{
    TapArgs64 t;
    const int last = 2 * L->order;
    for (int i = 0; i < 2 * PLX_MAX_ORDER + 1; ++i) t.c[i] = 0.0;
    for (int i = 0; i <= last; ++i) t.c[i] = (double)L->taps.c[mirrored ? last - i : i];
    return t;
}

int blur_t_f64_impl(plx_lattice *L, double *d_values, double *d_scratch, int vd, int *result_in_scratch, hipStream_t stream)
{
    const TapArgs64 taps = taps_f64(L, true);
    double *cur = d_values, *nxt = d_scratch;
    for (int a = L->d; a >= 0; --a) {
        blur_axis_f64(L, cur, nxt, a, vd, taps, stream);
        std::swap(cur, nxt);
    }
    *result_in_scratch = cur == d_scratch ? 1 : 0;
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

struct DualArgs {
    const double *fin, *rin;
    double *fout, *rout;
    const int *nbr_f, *nbr_r;
    bool first, last;
};

template <class V, int ORDER>
static void launch_dual_f64(plx_lattice *L, const DualArgs &a, int rowlen, const TapArgs64 &tf, const TapArgs64 &tr,
                            hipStream_t stream)
{
    const int m = (int)L->m;
    const int ntiles = ceil_div((int64_t)m * rowlen, kBlock);
    const V *fin = reinterpret_cast<const V *>(a.fin), *rin = reinterpret_cast<const V *>(a.rin);
    V *fout = reinterpret_cast<V *>(a.fout), *rout = reinterpret_cast<V *>(a.rout);
#define PLX_DUAL(FIRST, LAST)                                                                                        \
    f64_blur_dual_kernel<V, ORDER, FIRST, LAST><<<tile_grid(ntiles), kBlock, 0, stream>>>(                           \
        fin, rin, fout, rout, a.nbr_f, a.nbr_r, m, L->mstride, rowlen, L->order, tf, tr, ntiles)
    if (a.first && a.last) PLX_DUAL(true, true);
    else if (a.first) PLX_DUAL(true, false);
    else if (a.last) PLX_DUAL(false, true);
    else PLX_DUAL(false, false);
#undef PLX_DUAL
}

template <class V>
static void launch_dual_order_f64(plx_lattice *L, const DualArgs &a, int rowlen, const TapArgs64 &tf, const TapArgs64 &tr,
                                  hipStream_t stream)
{
    switch (L->order) {
    case 0: launch_dual_f64<V, 0>(L, a, rowlen, tf, tr, stream); break;
    case 1: launch_dual_f64<V, 1>(L, a, rowlen, tf, tr, stream); break;
    case 2: launch_dual_f64<V, 2>(L, a, rowlen, tf, tr, stream); break;
    case 3: launch_dual_f64<V, 3>(L, a, rowlen, tf, tr, stream); break;
    default: launch_dual_f64<V, -1>(L, a, rowlen, tf, tr, stream); break;
    }
}

int blur_sym_f64_planes(const plx_lattice *L) { return L->d + 1 >= 3 ? 3 : L->d + 1; }

int blur_sym_f64_impl(plx_lattice *L, double *d_values, double *const d_work[3], int vd, double **d_result, hipStream_t stream)
{
    const int d1 = L->d + 1, order = L->order;
    const int rowlen = vd == 1 ? 1 : values_stride_f64(vd) / 2;
    const TapArgs64 tf = taps_f64(L, false), tr = taps_f64(L, true);
    // the two plane pairs the launches alternate between: launch 0 reads d_values and writes pair A, launch 1 reads A and
    // writes B = (d_values, work 2), ...; the last launch writes the first plane of the pair it does not read
    double *pair[2][2] = {{d_work[0], d_work[1]}, {d_values, d_work[2]}};
    const double *fin = d_values, *rin = d_values;
    for (int k = 0; k < d1; ++k) {
        DualArgs a;
        a.first = k == 0;
        a.last = k == d1 - 1;
        a.fin = fin;
        a.rin = rin;
        a.fout = pair[k & 1][0];
        a.rout = a.last ? nullptr : pair[k & 1][1];
        a.nbr_f = L->nbr.as<int>() + (size_t)k * 2 * order * L->mstride;
        a.nbr_r = L->nbr.as<int>() + (size_t)(d1 - 1 - k) * 2 * order * L->mstride;
        if (vd == 1) launch_dual_order_f64<double>(L, a, rowlen, tf, tr, stream);
        else launch_dual_order_f64<double2>(L, a, rowlen, tf, tr, stream);
        fin = a.fout;
        rin = a.rout;
    }
    *d_result = const_cast<double *>(fin);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
