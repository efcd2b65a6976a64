// plx_kernels.h -- device helpers and launch-side switches shared by the per-MVM kernel files (plx_splat.hip,
// plx_blur.hip, plx_slice.hip, plx_block.hip, plx_first.hip, plx_onehot.hip, plx_f64.hip, plx_backward_f64.hip,
// through plx_rows_kernels.h plx_rows.hip and plx_rows_f64.hip, through plx_rows_backward_kernels.h plx_rows_backward.hip and
// plx_rows_backward_f64.hip, through plx_sym_kernels.h plx_sym.hip and plx_sym_f64.hip, through plx_diag_kernels.h
// plx_diag.hip and plx_diag_f64.hip, and through plx_query_kernels.h plx_query.hip and plx_query_f64.hip).  Not part of
// the C ABI.
//
// Reference: cpp/permutohedral.h ("h") splat value accumulation h:478-479,
// blur h:513-572, slice h:497-510.  The reference's CUDA path does the splat
// with one float atomicAdd per (point, corner, channel) and re-hashes every
// neighbour in every blur pass; here
//   gather-in  right-hand side rows into lattice point order (and, for vd > 1,
//              into rows padded to whole 16-byte vectors),
//   splat      segmented scan over simplex corners sorted by vertex (no
//              atomics, bitwise reproducible),
//   blur       d+1 gather-accumulate passes over a precomputed neighbour table,
//   slice      per-point gather through SoA (vertex id, weight) planes, result
//              scattered back to the caller's row order.
// All are HBM/cache-bandwidth bound gather stencils; no MFMA.
//
// Value rows: vd = 1 -> one float per vertex; vd > 1 -> vdp = roundup4(vd)
// floats, i.e. nch = vdp/4 float4 "chunks", and every access of the vector
// kernels is one aligned 16-byte load/store per lane.
#pragma once

#include "plx_internal.h"

#include <math.h>
#include <type_traits>

namespace plx {

// Diagnostic ablations (kernels with parts of their memory traffic switched off, for A/B profiles) exist only in
// libplx_diag.so (make diag: -DPLX_DIAG); in the shipped library the switches and the branches behind them are
// compiled out.
#ifdef PLX_DIAG
#define PLX_DIAG_VALUE(x) (x)
#else
#define PLX_DIAG_VALUE(x) 0
#endif

// kernel-variant switches (plx_tune); defined in plx_tune.hip and plx_build.hip

// Tile index for workgroup blockIdx.x.  With remap (every kernel but the two that measured faster in plain order and
// say so) the launch has 8 * ceil(ntiles / 8) workgroups and
// workgroup b takes tile (b % 8) * per + b / 8: workgroups are dealt to the 8 XCDs round-robin
// (MI355X_MICROARCH.md, Workgroup dispatch), so every XCD sweeps one contiguous eighth of the tiles and its
// gathers -- which follow the lattice order -- stay inside one eighth of the gathered array, i.e. inside
// its own 4 MiB L2.  Placement only affects speed, never results.  Returns -1 for the padding workgroups.
__device__ __forceinline__ int tile_index(int ntiles, int remap = 1)
{
    const int b = blockIdx.x;
    if (!remap) return b < ntiles ? b : -1;
    const int per = (ntiles + 7) >> 3;
    const int t = (b & 7) * per + (b >> 3);
    return ((b >> 3) < per && t < ntiles) ? t : -1;
}
static inline int tile_grid(int ntiles, int remap = 1) { return remap ? 8 * ((ntiles + 7) / 8) : ntiles; }

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4_scale(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ __forceinline__ float4 f4_sel(bool c, float4 a, float4 b) { return c ? a : b; }
__device__ __forceinline__ float4 f4_shfl_up(float4 a, int off)
{
    return make_float4(__shfl_up(a.x, off), __shfl_up(a.y, off), __shfl_up(a.z, off), __shfl_up(a.w, off));
}

// One scalar or one 16-byte chunk of a value row.  The double forms (the float64 product) have zero and fma only:
// fma(acc, s, x) is acc += s * x per element.
template <class V> struct VecOps;
template <> struct VecOps<float> {
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ float add(float a, float b) { return a + b; }
    static __device__ __forceinline__ float scale(float s, float a) { return s * a; }
    static __device__ __forceinline__ float sel(bool c, float a, float b) { return c ? a : b; }
    static __device__ __forceinline__ float shfl_up(float a, int off) { return __shfl_up(a, off); }
};
template <> struct VecOps<float4> {
    static __device__ __forceinline__ float4 zero() { return f4_zero(); }
    static __device__ __forceinline__ float4 add(float4 a, float4 b) { return f4_add(a, b); }
    static __device__ __forceinline__ float4 scale(float s, float4 a) { return f4_scale(s, a); }
    static __device__ __forceinline__ float4 sel(bool c, float4 a, float4 b) { return f4_sel(c, a, b); }
    static __device__ __forceinline__ float4 shfl_up(float4 a, int off) { return f4_shfl_up(a, off); }
};
template <> struct VecOps<double> {
    static __device__ __forceinline__ double zero() { return 0.0; }
    static __device__ __forceinline__ void fma(double &acc, double s, double x) { acc += s * x; }
};
template <> struct VecOps<double2> {
    static __device__ __forceinline__ double2 zero() { return make_double2(0.0, 0.0); }
    static __device__ __forceinline__ void fma(double2 &acc, double s, double2 x) { acc.x += s * x.x; acc.y += s * x.y; }
};

// ---- the float64 gathers (plx_f64.hip and, through Gather<double> below, the row-range product and the queries): the
// pieces all of them form their sums from, so that the same terms in the same order give the same bits in each ----
// one chunk of a caller row: a 16-byte access where the rows are whole aligned chunks, else per double with the tail guarded
template <bool VEC>
__device__ __forceinline__ double2 f64_load_chunk(const double *__restrict__ src, size_t row, int vd, int ch)
{
    const double *p = src + row * vd + 2 * ch;
    if constexpr (VEC) return *reinterpret_cast<const double2 *>(p);
    double2 x = VecOps<double2>::zero();
    x.x = p[0];
    if (vd - 2 * ch > 1) x.y = p[1];
    return x;
}

template <bool VEC>
__device__ __forceinline__ void f64_store_chunk(double *__restrict__ out, size_t row, int vd, int ch, double2 a)
{
    double *o = out + row * vd + 2 * ch;
    if constexpr (VEC) { *reinterpret_cast<double2 *>(o) = a; return; }
    o[0] = a.x;
    if (vd - 2 * ch > 1) o[1] = a.y;
}

// corners [j0, j1) of one vertex; csr_row carries the segment-head flag of the fp32 scan in its sign bit (a row-range
// table's rows have it clear)
template <bool VEC>
__device__ __forceinline__ double2 f64_vertex_sum(const int *__restrict__ row, const float *__restrict__ w, int j0, int j1,
                                                  const double *__restrict__ src, int vd, int ch)
{
    double2 acc = VecOps<double2>::zero();
    for (int j = j0; j < j1; ++j)
        VecOps<double2>::fma(acc, (double)w[j], f64_load_chunk<VEC>(src, (size_t)(row[j] & 0x7FFFFFFF), vd, ch));
    return acc;
}

// sum_r w_r values[v_r][ch] in corner order, then ONE division by 1 + 2^-d.  SKIP (the slices at located queries,
// plx_query_kernels.h): a corner whose id is negative is absent and contributes nothing -- skipped, not multiplied by zero;
// without it, the present behaviour: every id is a vertex.
template <bool SKIP = false>
__device__ __forceinline__ double2 f64_point_sum(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p,
                                                 int d1, const double2 *__restrict__ values, int nch, int ch, double denom)
{
    double2 acc = VecOps<double2>::zero();
    for (int r = 0; r < d1; ++r) {
        if constexpr (SKIP) {
            const int v = evid[(size_t)r * n + p];
            if (v < 0) continue;
            VecOps<double2>::fma(acc, (double)ew[(size_t)r * n + p], values[(size_t)v * nch + ch]);
        } else {
            VecOps<double2>::fma(acc, (double)ew[(size_t)r * n + p], values[(size_t)evid[(size_t)r * n + p] * nch + ch]);
        }
    }
    return make_double2(acc.x / denom, acc.y / denom);
}

// chunk ch of the filtered row of point p, the sum of the float64 chunk slices (f64_slice_chunk_kernel, the row-range and the
// query ones).  D1 > 0: d + 1 compiled in -- all ids, then all gathers, then the ordered sum with each weight converted where
// it is used, then ONE division; 0: the run-time form.  (filtered_chunk64 below reads its weights first: other registers.
// And the gather is spelled per SKIP: assigned from a conditional it is one 16-byte load, assigned directly two of 8.)
template <int D1, bool SKIP = false>
__device__ __forceinline__ double2 f64_filtered_chunk(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p,
                                                      int d1, const double2 *__restrict__ values, int nch, int ch, double denom)
{
    if constexpr (D1 > 0) {
        int v[D1];
        double2 g[D1];
#pragma unroll
        for (int r = 0; r < D1; ++r) v[r] = evid[(size_t)r * n + p];
#pragma unroll
        for (int r = 0; r < D1; ++r) {
            if constexpr (SKIP) g[r] = v[r] >= 0 ? values[(size_t)v[r] * nch + ch] : VecOps<double2>::zero();
            else g[r] = values[(size_t)v[r] * nch + ch];
        }
        double2 acc = VecOps<double2>::zero();
#pragma unroll
        for (int r = 0; r < D1; ++r)
            if (!SKIP || v[r] >= 0) VecOps<double2>::fma(acc, (double)ew[(size_t)r * n + p], g[r]);
        return make_double2(acc.x / denom, acc.y / denom);
    } else {
        return f64_point_sum<SKIP>(evid, ew, n, p, d1, values, nch, ch, denom);
    }
}

// ... and the vd = 1 sum of the same slices, in the same two forms
template <int D1, bool SKIP = false>
__device__ __forceinline__ double f64_filtered_v1(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p, int d1,
                                                  const double *__restrict__ values, double denom)
{
    double acc = 0.0;
    if constexpr (D1 > 0) {
        int v[D1];
        double g[D1];
#pragma unroll
        for (int r = 0; r < D1; ++r) v[r] = evid[(size_t)r * n + p];
#pragma unroll
        for (int r = 0; r < D1; ++r) g[r] = !SKIP || v[r] >= 0 ? values[v[r]] : 0.0;
#pragma unroll
        for (int r = 0; r < D1; ++r)
            if (!SKIP || v[r] >= 0) acc += (double)ew[(size_t)r * n + p] * g[r];
    } else {
        if constexpr (SKIP) {
            for (int r = 0; r < d1; ++r) {
                const int v = evid[(size_t)r * n + p];
                if (v < 0) continue;
                acc += (double)ew[(size_t)r * n + p] * values[v];
            }
        } else {
            for (int r = 0; r < d1; ++r) acc += (double)ew[(size_t)r * n + p] * values[evid[(size_t)r * n + p]];
        }
    }
    return acc / denom;
}

// ---- the float64 position gradients (plx_backward_f64.hip, plx_rows_backward_f64.hip): the stack formed inside the splat
// and the filtered row formed inside the slice, shared so that both files give the same bits ----
// One column of the stack: where its factor a comes from, and k >= 0 for a product column a * x[k] (-1: the plain column).
struct StackCol64 {
    const double *a;
    int l, k;
};

__device__ __forceinline__ StackCol64 stack_col64(int c, const double *__restrict__ g, const double *__restrict__ src, int L, int d)
{
    const int h = L * (1 + d);
    StackCol64 s;
    s.a = c < h ? g : src;
    if (c >= h) c -= h;
    if (c < L) {
        s.l = c;
        s.k = -1;
    } else {
        c -= L;
        s.l = c / d;
        s.k = c - s.l * d;
    }
    return s;
}

__device__ __forceinline__ double stack_elem64(const StackCol64 &s, const double *__restrict__ x, size_t row, int L, int d)
{
    const double a = s.a[row * L + s.l];
    return s.k < 0 ? a : a * x[row * d + s.k];
}

// f64_vertex_sum over chunk ch of the stack rows: the same weights, the same corner order, the same fma
__device__ __forceinline__ double2 stack_vertex_sum64(const int *__restrict__ row, const float *__restrict__ w, int j0, int j1,
                                                      const double *__restrict__ g, const double *__restrict__ src,
                                                      const double *__restrict__ x, int L, int d, int ch)
{
    const StackCol64 c0 = stack_col64(2 * ch, g, src, L, d), c1 = stack_col64(2 * ch + 1, g, src, L, d);
    double2 acc = VecOps<double2>::zero();
    for (int j = j0; j < j1; ++j) {
        const size_t r = (size_t)(row[j] & 0x7FFFFFFF);
        VecOps<double2>::fma(acc, (double)w[j], make_double2(stack_elem64(c0, x, r, L, d), stack_elem64(c1, x, r, L, d)));
    }
    return acc;
}

// The corners of point p, read once per lane.  D1 > 0: d + 1 compiled in; 0: nothing is kept, the run-time form reads them.
template <int D1> struct Corners64 {
    int v[D1];
    double w[D1];
    __device__ __forceinline__ void load(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p)
    {
#pragma unroll
        for (int r = 0; r < D1; ++r) v[r] = evid[(size_t)r * n + p];
#pragma unroll
        for (int r = 0; r < D1; ++r) w[r] = (double)ew[(size_t)r * n + p];
    }
};
template <> struct Corners64<0> {
    __device__ __forceinline__ void load(const int *, const float *, int, int) {}
};

// chunk ch of the filtered row of point p: the sum of f64_slice_chunk_kernel (all gathers, then the ordered sum, one division)
template <int D1>
__device__ __forceinline__ double2 filtered_chunk64(const Corners64<D1> &c, const int *__restrict__ evid, const float *__restrict__ ew,
                                                    int n, int p, int d1, const double2 *__restrict__ values, int nch, int ch,
                                                    double denom)
{
    if constexpr (D1 > 0) {
        double2 gath[D1];
#pragma unroll
        for (int r = 0; r < D1; ++r) gath[r] = values[(size_t)c.v[r] * nch + ch];
        double2 acc = VecOps<double2>::zero();
#pragma unroll
        for (int r = 0; r < D1; ++r) VecOps<double2>::fma(acc, c.w[r], gath[r]);
        return make_double2(acc.x / denom, acc.y / denom);
    } else {
        return f64_point_sum(evid, ew, n, p, d1, values, nch, ch, denom);
    }
}

// ---- the fp32 row-range slices (Gather<float> below, plx_rows_backward.hip): the sums both form a filtered chunk from, so
// that the same terms in the same order give the same bits in both ----
// acc += (w g) rden per element: the product w g rounded, then ONE fused multiply-add.  Written with the rounding spelled out:
// left to -ffp-contract=fast, `acc += w * g * rden` compiled to this in every kernel but the unaligned chunk slice, whose
// first column of each chunk the vectoriser paired across corners and left unfused, so that the bits of a product depended
// on the alignment of its output and no other kernel could promise them.
__device__ __forceinline__ void rows_term(float4 &acc, float w, float4 g, float rden)
{
    acc.x = __fmaf_rn(__fmul_rn(w, g.x), rden, acc.x);
    acc.y = __fmaf_rn(__fmul_rn(w, g.y), rden, acc.y);
    acc.z = __fmaf_rn(__fmul_rn(w, g.z), rden, acc.z);
    acc.w = __fmaf_rn(__fmul_rn(w, g.w), rden, acc.w);
}

// sum_r w_r values[v_r][ch] rden, in corner order, every term multiplied by the rounded reciprocal as plx_slice.hip does
// SKIP: as for f64_point_sum
template <bool SKIP = false>
__device__ __forceinline__ float4 rows_point_sum(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p,
                                                 int d1, const float4 *__restrict__ values, int nch, int ch, float rden)
{
    float4 acc = f4_zero();
    for (int r = 0; r < d1; ++r) {
        const int v = evid[(size_t)r * n + p];
        if constexpr (SKIP)
            if (v < 0) continue;
        const float wr = ew[(size_t)r * n + p];
        const float4 g = values[(size_t)v * nch + ch];
        rows_term(acc, wr, g, rden);
    }
    return acc;
}

// chunk ch of the filtered row of point p.  D1 > 0: d + 1 compiled in (all index / weight loads, then all gathers, then the
// ordered sum); 0: the run-time form
template <int D1, bool SKIP = false>
__device__ __forceinline__ float4 rows_filtered_chunk(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p,
                                                      int d1, const float4 *__restrict__ values, int nch, int ch, float rden)
{
    if constexpr (D1 > 0) {
        float4 acc = f4_zero();
        int v[D1];
        float wr[D1];
        float4 g[D1];
#pragma unroll
        for (int r = 0; r < D1; ++r) {
            v[r] = evid[(size_t)r * n + p];
            wr[r] = ew[(size_t)r * n + p];
        }
        if constexpr (SKIP) {
#pragma unroll
            for (int r = 0; r < D1; ++r) g[r] = v[r] >= 0 ? values[(size_t)v[r] * nch + ch] : f4_zero();
#pragma unroll
            for (int r = 0; r < D1; ++r)
                if (v[r] >= 0) rows_term(acc, wr[r], g[r], rden);
        } else {
#pragma unroll
            for (int r = 0; r < D1; ++r) g[r] = values[(size_t)v[r] * nch + ch];
#pragma unroll
            for (int r = 0; r < D1; ++r) rows_term(acc, wr[r], g[r], rden);
        }
        return acc;
    } else {
        return rows_point_sum<SKIP>(evid, ew, n, p, d1, values, nch, ch, rden);
    }
}

static inline bool f64_vec_ok(const void *p, int vd) { return (vd & 1) == 0 && ((uintptr_t)p & 15) == 0; }
// The chunk shape of the float64 kernels and of both row-range gradients: a group of 2^shift >= nch lanes per row, one lane
// per 16-byte chunk (float4 or double2), up to kChunkGroupMax chunks: a group never spans two waves.
constexpr int kChunkGroupMax = 64;
static inline int chunk_group_shift(int nch)
{
    int s = 0;
    while ((1 << s) < nch) ++s;
    return s;
}

// The gather slices of plx_rows_kernels.h, plx_query_kernels.h and plx_f64.hip have d + 1 compiled in up to kGatherMaxD1:
// f(std::integral_constant<int, D1>) with D1 = d1 for 2..20, else 0 (the run-time form).
constexpr int kGatherMaxD1 = 20;
template <class F> static inline void dispatch_d1(int d1, F &&f)
{
    switch (d1 <= kGatherMaxD1 ? d1 : 0) {
#define PLX_CASE(D1) case D1: f(std::integral_constant<int, D1>{}); break;
        PLX_CASE(2) PLX_CASE(3) PLX_CASE(4) PLX_CASE(5) PLX_CASE(6) PLX_CASE(7) PLX_CASE(8) PLX_CASE(9) PLX_CASE(10)
        PLX_CASE(11) PLX_CASE(12) PLX_CASE(13) PLX_CASE(14) PLX_CASE(15) PLX_CASE(16) PLX_CASE(17) PLX_CASE(18)
        PLX_CASE(19) PLX_CASE(20)
#undef PLX_CASE
    default: f(std::integral_constant<int, 0>{}); break;
    }
}

// ---- what the gathers of a caller type T differ in (the row-range product, plx_rows_kernels.h, and the slices at located
// queries, plx_query_kernels.h): the 16-byte chunk Vec, the normalisation Den, one chunk of a caller row (load / store: a
// 16-byte access where the rows are whole aligned chunks, else per element with the tail guarded), the sum over the corners
// of a vertex (vertex_sum) and the three sums over the corners of a point: v1 (vd = 1), chunk (d + 1 compiled in up to
// kGatherMaxD1) and wide.  Every sum is that type's own text: one body for both would change roundings or registers in one
// of them.  SKIP = false, the row-range product: every id is a vertex.  SKIP = true, the queries: (evid, ew) are the
// located (vid, w) with nq for n, and a corner whose id is negative is absent.  It is skipped, never multiplied by zero:
// the vertex array may hold non-finite values elsewhere.  With every corner present both give the same terms in the same
// order, hence the same bits.
template <typename T> struct Gather;

template <> struct Gather<float> {
    using Vec = float4;
    using Den = float;                        // the rounded reciprocal of 1 + 2^-d: every term is multiplied (rows_term)
    static constexpr int kPer = 4;            // elements per chunk
    static constexpr bool kV1Compiled = false;      // v1 reads its corners in a run-time loop
    static int stride(int vd) { return values_stride(vd); }
    static Den den(const plx_lattice *L) { return 1.0f / L->slice_denom; }
    static bool vec_ok(const void *p, int vd) { return (vd & 3) == 0 && ((uintptr_t)p & 15) == 0; }
    template <bool VEC> static __device__ __forceinline__ float4 load(const float *__restrict__ src, size_t row, int vd, int ch)
    {
        const float *p = src + row * vd + 4 * ch;
        if constexpr (VEC) return *reinterpret_cast<const float4 *>(p);
        const int left = vd - 4 * ch;
        float4 x = f4_zero();
        x.x = p[0];
        if (left > 1) x.y = p[1];
        if (left > 2) x.z = p[2];
        if (left > 3) x.w = p[3];
        return x;
    }
    template <bool VEC> static __device__ __forceinline__ void store(float *__restrict__ out, size_t row, int vd, int ch, float4 a)
    {
        float *o = out + row * vd + 4 * ch;
        if constexpr (VEC) { *reinterpret_cast<float4 *>(o) = a; return; }
        const int left = vd - 4 * ch;
        o[0] = a.x;
        if (left > 1) o[1] = a.y;
        if (left > 2) o[2] = a.z;
        if (left > 3) o[3] = a.w;
    }
    template <bool VEC>
    static __device__ __forceinline__ float4 vertex_sum(const int *__restrict__ row, const float *__restrict__ w, int j0, int j1,
                                                        const float *__restrict__ src, int vd, int ch)
    {
        float4 acc = f4_zero();
        for (int j = j0; j < j1; ++j) {
            const float wj = w[j];
            const float4 x = load<VEC>(src, (size_t)row[j], vd, ch);
            acc.x += wj * x.x; acc.y += wj * x.y; acc.z += wj * x.z; acc.w += wj * x.w;
        }
        return acc;
    }
    // the run-time loop (D1 is not used), each form as its kernel had it
    template <int D1, bool SKIP>
    static __device__ __forceinline__ float v1(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p, int d1,
                                               const float *__restrict__ values, float rden)
    {
        float acc = 0.f;
        if constexpr (SKIP) {
            for (int r = 0; r < d1; ++r) {
                const int v = evid[(size_t)r * n + p];
                if (v < 0) continue;
                acc += ew[(size_t)r * n + p] * values[v] * rden;
            }
        } else {
            for (int r = 0; r < d1; ++r) acc += ew[(size_t)r * n + p] * values[evid[(size_t)r * n + p]] * rden;
        }
        return acc;
    }
    template <int D1, bool SKIP>
    static __device__ __forceinline__ float4 chunk(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p, int d1,
                                                   const float4 *__restrict__ values, int nch, int ch, float rden)
    {
        return rows_filtered_chunk<D1, SKIP>(evid, ew, n, p, d1, values, nch, ch, rden);
    }
    template <bool SKIP>
    static __device__ __forceinline__ float4 wide(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p, int d1,
                                                  const float4 *__restrict__ values, int nch, int ch, float rden)
    {
        return rows_point_sum<SKIP>(evid, ew, n, p, d1, values, nch, ch, rden);
    }
};

template <> struct Gather<double> {
    using Vec = double2;
    using Den = double;                       // 1 + 2^-d itself: the double slices divide their sum once
    static constexpr int kPer = 2;
    static constexpr bool kV1Compiled = true;       // v1 has d + 1 compiled in
    static int stride(int vd) { return values_stride_f64(vd); }
    static Den den(const plx_lattice *L) { return 1.0 + ldexp(1.0, -L->d); }
    static bool vec_ok(const void *p, int vd) { return f64_vec_ok(p, vd); }
    template <bool VEC> static __device__ __forceinline__ double2 load(const double *__restrict__ src, size_t row, int vd, int ch)
    {
        return f64_load_chunk<VEC>(src, row, vd, ch);
    }
    template <bool VEC> static __device__ __forceinline__ void store(double *__restrict__ out, size_t row, int vd, int ch, double2 a)
    {
        f64_store_chunk<VEC>(out, row, vd, ch, a);
    }
    template <bool VEC>
    static __device__ __forceinline__ double2 vertex_sum(const int *__restrict__ row, const float *__restrict__ w, int j0, int j1,
                                                         const double *__restrict__ src, int vd, int ch)
    {
        return f64_vertex_sum<VEC>(row, w, j0, j1, src, vd, ch);
    }
    template <int D1, bool SKIP>
    static __device__ __forceinline__ double v1(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p, int d1,
                                                const double *__restrict__ values, double denom)
    {
        return f64_filtered_v1<D1, SKIP>(evid, ew, n, p, d1, values, denom);
    }
    template <int D1, bool SKIP>
    static __device__ __forceinline__ double2 chunk(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p,
                                                    int d1, const double2 *__restrict__ values, int nch, int ch, double denom)
    {
        return f64_filtered_chunk<D1, SKIP>(evid, ew, n, p, d1, values, nch, ch, denom);
    }
    template <bool SKIP>
    static __device__ __forceinline__ double2 wide(const int *__restrict__ evid, const float *__restrict__ ew, int n, int p,
                                                   int d1, const double2 *__restrict__ values, int nch, int ch, double denom)
    {
        return f64_point_sum<SKIP>(evid, ew, n, p, d1, values, nch, ch, denom);
    }
};

}  // namespace plx
