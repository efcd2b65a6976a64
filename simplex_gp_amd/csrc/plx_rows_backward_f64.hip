// plx_rows_backward_f64.hip -- the float64 one-sided position gradient of the rectangular product
// (plx_backward_splat_rows_f64 / plx_backward_contract_rows_f64 / plx_apply_backward_rows_f64):
// plx_rows_backward_kernels.h with T = double.  The kernels, the contraction and the launch side are there; here is what
// float64 rounds in its own way, over the pieces of plx_kernels.h it shares with the square gradient (plx_backward_f64.hip),
// and the names it reports.

#include "plx_rows_backward_kernels.h"

#include <math.h>

namespace plx {

template <> struct RowsBackward<double> : RowsBackwardHost<double> {
    using Chunk = double2;
    template <int D1> using Corners = Corners64<D1>;      // the corners of a point, read once per lane

    static constexpr const char *plx_lattice::*kSplatField = &plx_lattice::kn_rows64_splat;
    static constexpr const char *plx_lattice::*kSliceField = &plx_lattice::kn_rows64_slice;
    static constexpr const char *kSplatChunk = "rows64_backward_splat_chunk_kernel";
    static constexpr const char *kSplatWide = "rows64_backward_splat_wide_kernel";
    static constexpr const char *kContractChunk = "rows64_backward_contract_chunk_kernel";
    static constexpr const char *kContractWide = "rows64_backward_contract_wide_kernel";

    // stack_vertex_sum64 over chunk ch of the HALF stack [ a | a (x) x ]: both halves of the square stack's column decoder
    // point at a, so every column c < H decodes as the square stack's column c; the padding column of an odd H is set to 0
    static __device__ __forceinline__ double2 half_stack_vertex_sum(const int *__restrict__ row, const float *__restrict__ w, int j0,
                                                                    int j1, const double *__restrict__ a,
                                                                    const double *__restrict__ x, int L, int d, int ch)
    {
        double2 acc = stack_vertex_sum64(row, w, j0, j1, a, a, x, L, d, ch);
        if (2 * ch + 1 >= L * (1 + d)) acc.y = 0.0;
        return acc;
    }

    // the sums of the slice are divided ONCE, by 1 + 2^-d
    static double slice_scale(const plx_lattice *L) { return 1.0 + ldexp(1.0, -L->d); }

    template <int D1>
    static __device__ __forceinline__ double2 filtered_chunk(const Corners64<D1> &c, const int *__restrict__ evid,
                                                             const float *__restrict__ ew, int n, int p, int d1,
                                                             const double2 *__restrict__ values, int nch, int ch, double denom)
    {
        return filtered_chunk64<D1>(c, evid, ew, n, p, d1, values, nch, ch, denom);
    }
};

template int backward_rows_tables<double>(plx_lattice *, int64_t, int64_t, int64_t, int64_t, hipStream_t);
template int backward_splat_rows_impl<double>(plx_lattice *, const double *, int64_t, int64_t, const double *, int, double *,
                                              hipStream_t);
template int backward_contract_rows_impl<double>(plx_lattice *, const double *, const double *, int64_t, int64_t, const double *,
                                                 int, double *, double *, hipStream_t);

}  // namespace plx
