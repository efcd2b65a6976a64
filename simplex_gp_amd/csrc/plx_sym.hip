// plx_sym.hip -- the transposed and the symmetrised fp32 blur on a built lattice: plx_blur_t / plx_blur_sym and the
// products around them (include/plx.h; the entry points and their argument checks are in plx_api.hip).  The fp32
// counterpart of plx_sym_f64.hip, which explains the construction:
//   K^T = S B'_0 ... B'_d S^T / (1 + 2^-d)   the axes in reverse order with mirrored taps c'[i] = c[2 r - i] -- host code
//         around blur_axis_kernel, the general family of plx_blur.hip (blur_axis_general), one launch per axis;
//   K_s = (K + K^T) / 2 = S (B_fwd + B_rev) / 2 S^T / (1 + 2^-d)   one splat, two blur chains, one slice.
//
// blur_dual_kernel advances both chains in one launch: launch k of d + 1 takes the forward chain F through axis k and the
// reverse chain R through axis d - k.  One thread per (vertex, 16-byte chunk), all 4 r neighbour ids in flight, then all
// 4 r gathers and the two centres, then each chain's sum in blur_axis_kernel's slot order and expression forms (lower
// slots, centre, upper slots; acc = add(acc, scale(c, x)); an absent neighbour skipped) -- so F and R hold, launch by
// launch, the bits the general family of plx_blur and plx_blur_t hold after as many axes.
//   FIRST  both chains read the one splat plane (no copy);
//   LAST   the launch stores the single plane 0.5f (F + R): one rounded sum, the halving exact;
//   k == d - k (the middle launch of an even d): both chains gather through the same ids, loaded once.
// Planes: F and R are SEPARATE planes of m rows (plx_sym_f64.hip says why).  Four planes in all (d_values + three of
// work): a launch reads one pair and writes the other, so no thread stores where another still gathers; the last launch
// writes a plane of the pair it does not read.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, no LDS, bitwise
// reproducible.

#include "plx_kernels.h"

#include <utility>

namespace plx {

// One chain's sum over one axis: blur_axis_kernel's, from ids and gathers already in registers.
template <class V, int ORDER>
__device__ __forceinline__ V dual_sum(const int (&id)[2 * ORDER + 1], const V (&g)[2 * ORDER + 1], V centre, const float *c)
{
    using O = VecOps<V>;
    V acc = O::zero();
#pragma unroll
    for (int s = 0; s < ORDER; ++s)
        if (id[s] >= 0) acc = O::add(acc, O::scale(c[s], g[s]));
    acc = O::add(acc, O::scale(c[ORDER], centre));
#pragma unroll
    for (int s = 0; s < ORDER; ++s)
        if (id[ORDER + s] >= 0) acc = O::add(acc, O::scale(c[ORDER + 1 + s], g[ORDER + s]));
    return acc;
}

// ... and its run-time form (ORDER = -1): blur_axis_kernel's loop
template <class V>
__device__ __forceinline__ V dual_sum_rt(const V *__restrict__ old, const int *__restrict__ nbr, int64_t mstride, uint32_t i,
                                         uint32_t ch, uint32_t item, uint32_t rowlen, int order, const float *c)
{
    using O = VecOps<V>;
    V acc = O::zero();
    for (int s = 0; s < order; ++s) {
        const int nb = nbr[s * mstride + i];
        if (nb >= 0) acc = O::add(acc, O::scale(c[s], old[(uint32_t)nb * rowlen + ch]));
    }
    acc = O::add(acc, O::scale(c[order], old[item]));
    for (int s = 0; s < order; ++s) {
        const int nb = nbr[(order + s) * mstride + i];
        if (nb >= 0) acc = O::add(acc, O::scale(c[order + 1 + s], old[(uint32_t)nb * rowlen + ch]));
    }
    return acc;
}

// 0.5f (f + r): the sum rounded once on its own (never contracted with what formed f or r), the halving exact
__device__ __forceinline__ float half_sum(float f, float r)
{
#pragma clang fp contract(off)
    const float s = f + r;
    return 0.5f * s;
}
__device__ __forceinline__ float dual_mean(float f, float r) { return half_sum(f, r); }
__device__ __forceinline__ float4 dual_mean(float4 f, float4 r)
{
    return make_float4(half_sum(f.x, r.x), half_sum(f.y, r.y), half_sum(f.z, r.z), half_sum(f.w, r.w));
}

// V = float (vd = 1, rowlen 1) or float4 (rowlen chunks per vertex).  ORDER >= 0: compiled in; -1: order_rt.
// fin / rin: the planes the two chains read (FIRST: rin is not read, both read fin); fout / rout: the planes they write
// (LAST: fout receives 0.5f (F + R), rout is not written).  nbr_f / nbr_r: the neighbour tables of axis k and axis d - k.
// No plane is __restrict__: with FIRST both chains read the same one.
template <class V, int ORDER, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBlock) void blur_dual_kernel(const V *fin, const V *rin, V *fout, V *rout,
                                                           const int *__restrict__ nbr_f, const int *__restrict__ nbr_r, int m,
                                                           int64_t mstride, int rowlen_, int order_rt, TapArgs taps_f,
                                                           TapArgs taps_r, int ntiles)
{
    const int tile = tile_index(ntiles);
    if (tile < 0) return;
    const uint32_t rowlen = (uint32_t)rowlen_;
    const uint32_t item = (uint32_t)tile * kBlock + threadIdx.x;      // (the entry point checks m * rowlen < 2^31)
    if (item >= (uint32_t)m * rowlen) return;
    const uint32_t i = item / rowlen, ch = item - i * rowlen;
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
        for (int s = 0; s < 2 * ORDER; ++s) gf[s] = fin[idf[s] >= 0 ? (uint32_t)idf[s] * rowlen + ch : item];
#pragma unroll
        for (int s = 0; s < 2 * ORDER; ++s) gr[s] = rsrc[idr[s] >= 0 ? (uint32_t)idr[s] * rowlen + ch : item];
        const V cf = fin[item];
        const V cr = FIRST ? cf : rsrc[item];
        f = dual_sum<V, ORDER>(idf, gf, cf, taps_f.c);
        r = dual_sum<V, ORDER>(idr, gr, cr, taps_r.c);
    } else {
        f = dual_sum_rt<V>(fin, nbr_f, mstride, i, ch, item, rowlen, order_rt, taps_f.c);
        r = dual_sum_rt<V>(rsrc, nbr_r, mstride, i, ch, item, rowlen, order_rt, taps_r.c);
    }
    if constexpr (LAST) {
        fout[item] = dual_mean(f, r);
    } else {
        fout[item] = f;
        rout[item] = r;
    }
}

// ---- launch side ---------------------------------------------------------------------------------------------------
static TapArgs taps_of(const plx_lattice *L, bool mirrored)
{
    TapArgs t;
    const int last = 2 * L->order;
    for (int i = 0; i < 2 * PLX_MAX_ORDER + 1; ++i) t.c[i] = 0.f;
    for (int i = 0; i <= last; ++i) t.c[i] = L->taps.c[mirrored ? last - i : i];
    return t;
}

int blur_t_impl(plx_lattice *L, float *d_values, float *d_scratch, int vd, int *result_in_scratch, hipStream_t stream)
{
    const TapArgs taps = taps_of(L, true);
    float *cur = d_values, *nxt = d_scratch;
    for (int a = L->d; a >= 0; --a) {
        blur_axis_general(L, cur, nxt, a, vd, taps, stream);
        std::swap(cur, nxt);
    }
    *result_in_scratch = cur == d_scratch ? 1 : 0;
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

struct DualArgs {
    const float *fin, *rin;
    float *fout, *rout;
    const int *nbr_f, *nbr_r;
    bool first, last;
};

template <class V, int ORDER>
static void launch_dual(plx_lattice *L, const DualArgs &a, int rowlen, const TapArgs &tf, const TapArgs &tr, hipStream_t stream)
{
    const int m = (int)L->m;
    const int ntiles = ceil_div((int64_t)m * rowlen, kBlock);
    const V *fin = reinterpret_cast<const V *>(a.fin), *rin = reinterpret_cast<const V *>(a.rin);
    V *fout = reinterpret_cast<V *>(a.fout), *rout = reinterpret_cast<V *>(a.rout);
#define PLX_DUAL(FIRST, LAST)                                                                                        \
    blur_dual_kernel<V, ORDER, FIRST, LAST><<<tile_grid(ntiles), kBlock, 0, stream>>>(                               \
        fin, rin, fout, rout, a.nbr_f, a.nbr_r, m, L->mstride, rowlen, L->order, tf, tr, ntiles)
    if (a.first && a.last) PLX_DUAL(true, true);
    else if (a.first) PLX_DUAL(true, false);
    else if (a.last) PLX_DUAL(false, true);
    else PLX_DUAL(false, false);
#undef PLX_DUAL
}

template <class V>
static void launch_dual_order(plx_lattice *L, const DualArgs &a, int rowlen, const TapArgs &tf, const TapArgs &tr,
                              hipStream_t stream)
{
    switch (L->order) {
    case 0: launch_dual<V, 0>(L, a, rowlen, tf, tr, stream); break;
    case 1: launch_dual<V, 1>(L, a, rowlen, tf, tr, stream); break;
    case 2: launch_dual<V, 2>(L, a, rowlen, tf, tr, stream); break;
    case 3: launch_dual<V, 3>(L, a, rowlen, tf, tr, stream); break;
    default: launch_dual<V, -1>(L, a, rowlen, tf, tr, stream); break;
    }
}

int blur_sym_planes(const plx_lattice *L) { return L->d + 1 >= 3 ? 3 : L->d + 1; }

int blur_sym_impl(plx_lattice *L, float *d_values, float *const d_work[3], int vd, float **d_result, hipStream_t stream)
{
    const int d1 = L->d + 1, order = L->order;
    const int rowlen = vd == 1 ? 1 : values_stride(vd) / 4;
    if ((int64_t)L->m * rowlen >= (1ll << 31)) {
        set_error("blur_sym: %lld vertices x %d columns exceed the 31-bit element index of the blur kernels", (long long)L->m, vd);
        return PLX_ERR_TOO_LARGE;
    }
    const TapArgs tf = taps_of(L, false), tr = taps_of(L, true);
    // the two plane pairs the launches alternate between: launch 0 reads d_values and writes pair A, launch 1 reads A and
    // writes B = (d_values, work 2), ...; the last launch writes the first plane of the pair it does not read
    float *pair[2][2] = {{d_work[0], d_work[1]}, {d_values, d_work[2]}};
    const float *fin = d_values, *rin = d_values;
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
        if (vd == 1) launch_dual_order<float>(L, a, rowlen, tf, tr, stream);
        else launch_dual_order<float4>(L, a, rowlen, tf, tr, stream);
        fin = a.fout;
        rin = a.rout;
    }
    *d_result = const_cast<float *>(fin);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
