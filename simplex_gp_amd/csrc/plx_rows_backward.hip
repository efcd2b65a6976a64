// plx_rows_backward.hip -- the fp32 one-sided position gradient of the rectangular product (plx_backward_splat_rows /
// plx_backward_contract_rows / plx_apply_backward_rows): plx_rows_backward_kernels.h with T = float.  The kernels, the
// contraction and the launch side are there; here is what fp32 rounds in its own way, with the conventions of plx_rows.hip,
// and the names it reports.

#include "plx_rows_backward_kernels.h"

namespace plx {

// One column of the half stack, decoded once per lane: l, and k >= 0 for a product column a_l * x_k, -1 for the plain column
// a_l, -2 for a padding column.
struct HalfCol {
    int l, k;
};

__device__ __forceinline__ HalfCol half_col(int c, int L, int d)
{
    HalfCol s;
    if (c >= L * (1 + d)) {
        s.l = 0;
        s.k = -2;
    } else if (c < L) {
        s.l = c;
        s.k = -1;
    } else {
        c -= L;
        s.l = c / d;
        s.k = c - s.l * d;
    }
    return s;
}

__device__ __forceinline__ float half_elem(const HalfCol &s, const float *__restrict__ a, const float *__restrict__ x, size_t row,
                                           int L, int d)
{
    if (s.k == -2) return 0.f;
    const float al = a[row * L + s.l];
    return s.k < 0 ? al : __fmul_rn(al, x[row * d + s.k]);
}

template <> struct RowsBackward<float> : RowsBackwardHost<float> {
    using Chunk = float4;
    // rows_filtered_chunk reads the corners of its point itself, per chunk
    template <int D1> struct Corners {
        __device__ __forceinline__ void load(const int *, const float *, int, int) {}
    };

    static constexpr const char *plx_lattice::*kSplatField = &plx_lattice::kn_rows_splat;
    static constexpr const char *plx_lattice::*kSliceField = &plx_lattice::kn_rows_slice;
    static constexpr const char *kSplatChunk = "rows_backward_splat_chunk_kernel";
    static constexpr const char *kSplatWide = "rows_backward_splat_wide_kernel";
    static constexpr const char *kContractChunk = "rows_backward_contract_chunk_kernel";
    static constexpr const char *kContractWide = "rows_backward_contract_wide_kernel";

    // Gather<float>::vertex_sum over chunk ch of the half stack rows: the same weights, the same corner order, the same expression
    static __device__ __forceinline__ float4 half_stack_vertex_sum(const int *__restrict__ row, const float *__restrict__ w, int j0,
                                                                   int j1, const float *__restrict__ a, const float *__restrict__ x,
                                                                   int L, int d, int ch)
    {
        const HalfCol c0 = half_col(4 * ch, L, d), c1 = half_col(4 * ch + 1, L, d), c2 = half_col(4 * ch + 2, L, d),
                      c3 = half_col(4 * ch + 3, L, d);
        float4 acc = f4_zero();
        for (int j = j0; j < j1; ++j) {
            const float wj = w[j];
            const size_t r = (size_t)row[j];
            const float4 e = make_float4(half_elem(c0, a, x, r, L, d), half_elem(c1, a, x, r, L, d), half_elem(c2, a, x, r, L, d),
                                         half_elem(c3, a, x, r, L, d));
            acc.x += wj * e.x; acc.y += wj * e.y; acc.z += wj * e.z; acc.w += wj * e.w;
        }
        return acc;
    }

    // every term of the slice is multiplied by the rounded reciprocal, as plx_slice.hip does
    static float slice_scale(const plx_lattice *L) { return 1.0f / L->slice_denom; }

    template <int D1>
    static __device__ __forceinline__ float4 filtered_chunk(const Corners<D1> &, const int *__restrict__ evid,
                                                            const float *__restrict__ ew, int n, int p, int d1,
                                                            const float4 *__restrict__ values, int nch, int ch, float rden)
    {
        return rows_filtered_chunk<D1>(evid, ew, n, p, d1, values, nch, ch, rden);
    }
};

template int backward_rows_tables<float>(plx_lattice *, int64_t, int64_t, int64_t, int64_t, hipStream_t);
template int backward_splat_rows_impl<float>(plx_lattice *, const float *, int64_t, int64_t, const float *, int, float *,
                                             hipStream_t);
template int backward_contract_rows_impl<float>(plx_lattice *, const float *, const float *, int64_t, int64_t, const float *, int,
                                                float *, float *, hipStream_t);

}  // namespace plx
