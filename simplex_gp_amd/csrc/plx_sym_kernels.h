// plx_sym_kernels.h -- the transposed and the symmetrised blur on a built lattice, in fp32 and in float64: plx_blur_t /
// plx_blur_sym, the same two with _f64 and the products around them (include/plx.h; the entry points and their argument
// checks are in plx_api.hip).  One templated source, instantiated by plx_sym.hip (float) and plx_sym_f64.hip (double): each
// holds the trait Sym<T> of its type and the *_impl / *_planes functions plx_internal.h declares, as one-line forwards.
//
// The operator K = S B_d ... B_0 S^T / (1 + 2^-d) is not symmetric: the d + 1 axis blurs do not commute.  On a plain
// build the neighbour table is symmetric (u is the +j neighbour of v exactly when v is the -j neighbour of u), so the
// transpose of one axis blur is the same axis with the taps mirrored, c'[i] = c[2 r - i], and
//   K^T = S B'_0 ... B'_d S^T / (1 + 2^-d):  the axes in reverse order, mirrored taps -- host code (sym_blur_t) around the
//         single-axis blur of the type, one launch per axis, nothing new on the device;
//   K_s = (K + K^T) / 2 = S  (B_fwd + B_rev) / 2  S^T / (1 + 2^-d):  one splat, two blur chains, one slice.
//
// blur_dual_kernel advances both chains in one launch: launch k of d + 1 takes the forward chain F through axis k and the
// reverse chain R through axis d - k.  One thread per (vertex, 16-byte chunk), all 4 r neighbour ids in flight, then all
// 4 r gathers and the two centres, then each chain's sum in the slot order and the expression forms of the type's
// single-axis blur (lower slots, centre, upper slots; an absent neighbour skipped) -- so F and R hold, launch by launch,
// the bits the plain blur's general kernels and the transposed blur hold after as many axes.
//   FIRST  both chains read the one splat plane (no copy);
//   LAST   the launch stores the single plane 0.5 (F + R): one rounded sum, the halving exact;
//   k == d - k (the middle launch of an even d): both chains gather through the same ids, loaded once.
// Planes: F and R are SEPARATE planes of m rows, not interleaved rows.  A chain's gathers follow the lattice order along
// one axis, and tile_index keeps every XCD inside one eighth of the plane it gathers from; rows interleaved [F | R] would
// double the stride between the rows one chain gathers -- half of every fetched line (float64, vd = 1: 8 useful bytes in
// 16) the other chain's, which gathers along another axis -- and halve what an XCD's L2 holds of either.  Four planes in
// all (d_values + three of work): a launch reads one pair and writes the other, so no thread stores where another still
// gathers; the last launch writes a plane of the pair it does not read.
// Every output element is written by exactly one thread from sums in a fixed order: no atomics, no LDS, bitwise
// reproducible.
//
// What the types differ in, all of it in Sym<T>:
//   float:  V1 / VN = float / float4 (kPack = 4 elements, values_stride), TapArgs.  One term is acc = add(acc, scale(c, x)),
//           blur_axis_kernel's; gathers are indexed in uint32_t and rowlen is held as uint32_t (the entry points check
//           m * stride < 2^31).  The transposed blur wraps blur_axis_general, the general family of plx_blur.hip.
//   double: V1 / VN = double / double2 (kPack = 2, values_stride_f64), TapArgs64.  One term is VecOps::fma(acc, c, x),
//           f64_blur_item's; gathers are indexed in size_t and rowlen stays an int.  The transposed blur wraps
//           blur_axis_f64 of plx_f64.hip.
// The index and rowlen types are what each type's kernels were compiled from before the two sources became one, and keep
// their machine code what it was.  The kernels report as blur_dual_kernel (plx_last_sym_kernels) and f64_blur_dual_kernel
// (plx_last_sym_f64_kernels); the symbols a profiler shows are blur_dual_kernel<float, ...> and blur_dual_kernel<double, ...>.
#pragma once
#include "plx_kernels.h"

#include <utility>

namespace plx {

// V1, VN, Taps, Index, Rowlen, kPack, stride(), term(), axis()
template <class T> struct Sym;

// One chain's sum over one axis: the single-axis blur's, from ids and gathers already in registers.
template <class T, class V, int ORDER>
__device__ __forceinline__ V dual_sum(const int (&id)[2 * ORDER + 1], const V (&g)[2 * ORDER + 1], V centre, const T *c)
{
    V acc = VecOps<V>::zero();
#pragma unroll
    for (int s = 0; s < ORDER; ++s)
        if (id[s] >= 0) Sym<T>::term(acc, c[s], g[s]);
    Sym<T>::term(acc, c[ORDER], centre);
#pragma unroll
    for (int s = 0; s < ORDER; ++s)
        if (id[ORDER + s] >= 0) Sym<T>::term(acc, c[ORDER + 1 + s], g[ORDER + s]);
    return acc;
}

// ... and its run-time form (ORDER = -1): the single-axis blur's loop
template <class T, class V>
__device__ __forceinline__ V dual_sum_rt(const V *__restrict__ old, const int *__restrict__ nbr, int64_t mstride, uint32_t i,
                                         uint32_t ch, uint32_t item, typename Sym<T>::Rowlen rowlen, int order, const T *c)
{
    using I = typename Sym<T>::Index;
    V acc = VecOps<V>::zero();
    for (int s = 0; s < order; ++s) {
        const int nb = nbr[s * mstride + i];
        if (nb >= 0) Sym<T>::term(acc, c[s], old[(I)nb * rowlen + ch]);
    }
    Sym<T>::term(acc, c[order], old[item]);
    for (int s = 0; s < order; ++s) {
        const int nb = nbr[(order + s) * mstride + i];
        if (nb >= 0) Sym<T>::term(acc, c[order + 1 + s], old[(I)nb * rowlen + ch]);
    }
    return acc;
}

// 0.5 (f + r): the sum rounded once on its own (never contracted with what formed f or r), the halving exact
template <class T> __device__ __forceinline__ T half_sum(T f, T r)
{
#pragma clang fp contract(off)
    const T s = f + r;
    return (T)0.5 * s;
}
__device__ __forceinline__ float dual_mean(float f, float r) { return half_sum(f, r); }
__device__ __forceinline__ double dual_mean(double f, double r) { return half_sum(f, r); }
__device__ __forceinline__ float4 dual_mean(float4 f, float4 r)
{
    return make_float4(half_sum(f.x, r.x), half_sum(f.y, r.y), half_sum(f.z, r.z), half_sum(f.w, r.w));
}
__device__ __forceinline__ double2 dual_mean(double2 f, double2 r) { return make_double2(half_sum(f.x, r.x), half_sum(f.y, r.y)); }

// V = V1 (vd = 1, rowlen 1) or VN (rowlen chunks per vertex).  ORDER >= 0: compiled in; -1: order_rt.
// fin / rin: the planes the two chains read (FIRST: rin is not read, both read fin); fout / rout: the planes they write
// (LAST: fout receives 0.5 (F + R), rout is not written).  nbr_f / nbr_r: the neighbour tables of axis k and axis d - k.
// No plane is __restrict__: with FIRST both chains read the same one.
template <class T, class V, int ORDER, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBlock) void blur_dual_kernel(const V *fin, const V *rin, V *fout, V *rout,
                                                           const int *__restrict__ nbr_f, const int *__restrict__ nbr_r, int m,
                                                           int64_t mstride, int rowlen_, int order_rt,
                                                           typename Sym<T>::Taps taps_f, typename Sym<T>::Taps taps_r, int ntiles)
{
    using I = typename Sym<T>::Index;
    const int tile = tile_index(ntiles);
    if (tile < 0) return;
    const typename Sym<T>::Rowlen rowlen = (typename Sym<T>::Rowlen)rowlen_;
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
        for (int s = 0; s < 2 * ORDER; ++s) gf[s] = fin[idf[s] >= 0 ? (I)idf[s] * rowlen + ch : (I)item];
#pragma unroll
        for (int s = 0; s < 2 * ORDER; ++s) gr[s] = rsrc[idr[s] >= 0 ? (I)idr[s] * rowlen + ch : (I)item];
        const V cf = fin[item];
        const V cr = FIRST ? cf : rsrc[item];
        f = dual_sum<T, V, ORDER>(idf, gf, cf, taps_f.c);
        r = dual_sum<T, V, ORDER>(idr, gr, cr, taps_r.c);
    } else {
        f = dual_sum_rt<T, V>(fin, nbr_f, mstride, i, ch, item, rowlen, order_rt, taps_f.c);
        r = dual_sum_rt<T, V>(rsrc, nbr_r, mstride, i, ch, item, rowlen, order_rt, taps_r.c);
    }
    if constexpr (LAST) {
        fout[item] = dual_mean(f, r);
    } else {
        fout[item] = f;
        rout[item] = r;
    }
}

// ---- launch side ---------------------------------------------------------------------------------------------------
template <class T> typename Sym<T>::Taps sym_taps(const plx_lattice *L, bool mirrored)
{
    typename Sym<T>::Taps t;
    const int last = 2 * L->order;
    for (int i = 0; i < 2 * PLX_MAX_ORDER + 1; ++i) t.c[i] = 0;
    for (int i = 0; i <= last; ++i) t.c[i] = (T)L->taps.c[mirrored ? last - i : i];
    return t;
}

template <class T> int sym_blur_t(plx_lattice *L, T *d_values, T *d_scratch, int vd, int *result_in_scratch, hipStream_t stream)
{
    const typename Sym<T>::Taps taps = sym_taps<T>(L, true);
    T *cur = d_values, *nxt = d_scratch;
    for (int a = L->d; a >= 0; --a) {
        Sym<T>::axis(L, cur, nxt, a, vd, taps, stream);
        std::swap(cur, nxt);
    }
    *result_in_scratch = cur == d_scratch ? 1 : 0;
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <class T> struct DualArgs {
    const T *fin, *rin;
    T *fout, *rout;
    const int *nbr_f, *nbr_r;
    bool first, last;
    typename Sym<T>::Taps taps_f, taps_r;
};

template <class T, class V, int ORDER> void launch_dual(plx_lattice *L, const DualArgs<T> &a, int rowlen, hipStream_t stream)
{
    const int m = (int)L->m;
    const int ntiles = ceil_div((int64_t)m * rowlen, kBlock);
    const V *fin = reinterpret_cast<const V *>(a.fin), *rin = reinterpret_cast<const V *>(a.rin);
    V *fout = reinterpret_cast<V *>(a.fout), *rout = reinterpret_cast<V *>(a.rout);
#define PLX_DUAL(FIRST, LAST)                                                                                        \
    blur_dual_kernel<T, V, ORDER, FIRST, LAST><<<tile_grid(ntiles), kBlock, 0, stream>>>(                            \
        fin, rin, fout, rout, a.nbr_f, a.nbr_r, m, L->mstride, rowlen, L->order, a.taps_f, a.taps_r, ntiles)
    if (a.first && a.last) PLX_DUAL(true, true);
    else if (a.first) PLX_DUAL(true, false);
    else if (a.last) PLX_DUAL(false, true);
    else PLX_DUAL(false, false);
#undef PLX_DUAL
}

template <class T, class V> void launch_dual_order(plx_lattice *L, const DualArgs<T> &a, int rowlen, hipStream_t stream)
{
    switch (L->order) {
    case 0: launch_dual<T, V, 0>(L, a, rowlen, stream); break;
    case 1: launch_dual<T, V, 1>(L, a, rowlen, stream); break;
    case 2: launch_dual<T, V, 2>(L, a, rowlen, stream); break;
    case 3: launch_dual<T, V, 3>(L, a, rowlen, stream); break;
    default: launch_dual<T, V, -1>(L, a, rowlen, stream); break;
    }
}

inline int sym_planes(const plx_lattice *L) { return L->d + 1 >= 3 ? 3 : L->d + 1; }

template <class T> int sym_blur(plx_lattice *L, T *d_values, T *const d_work[3], int vd, T **d_result, hipStream_t stream)
{
    const int d1 = L->d + 1, order = L->order;
    const int rowlen = vd == 1 ? 1 : Sym<T>::stride(vd) / Sym<T>::kPack;
    DualArgs<T> a;
    a.taps_f = sym_taps<T>(L, false);
    a.taps_r = sym_taps<T>(L, true);
    // the two plane pairs the launches alternate between: launch 0 reads d_values and writes pair A, launch 1 reads A and
    // writes B = (d_values, work 2), ...; the last launch writes the first plane of the pair it does not read
    T *pair[2][2] = {{d_work[0], d_work[1]}, {d_values, d_work[2]}};
    const T *fin = d_values, *rin = d_values;
    for (int k = 0; k < d1; ++k) {
        a.first = k == 0;
        a.last = k == d1 - 1;
        a.fin = fin;
        a.rin = rin;
        a.fout = pair[k & 1][0];
        a.rout = a.last ? nullptr : pair[k & 1][1];
        a.nbr_f = L->nbr.as<int>() + (size_t)k * 2 * order * L->mstride;
        a.nbr_r = L->nbr.as<int>() + (size_t)(d1 - 1 - k) * 2 * order * L->mstride;
        if (vd == 1) launch_dual_order<T, typename Sym<T>::V1>(L, a, rowlen, stream);
        else launch_dual_order<T, typename Sym<T>::VN>(L, a, rowlen, stream);
        fin = a.fout;
        rin = a.rout;
    }
    *d_result = const_cast<T *>(fin);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
