// plx_sym_f64.hip -- the transposed and the symmetrised float64 blur on a built lattice (plx_blur_t_f64 / plx_blur_sym_f64
// and the products around them): plx_sym_kernels.h with T = double.  The kernel and the launch side are there; here is what
// float64 does in its own way.

#include "plx_sym_kernels.h"

namespace plx {

template <> struct Sym<double> {
    using V1 = double;
    using VN = double2;
    using Taps = TapArgs64;
    using Index = size_t;      // of a gather
    using Rowlen = int;
    static constexpr int kPack = 2;
    static int stride(int vd) { return values_stride_f64(vd); }
    // f64_blur_item's term: one fma
    template <class V> static __device__ __forceinline__ void term(V &acc, double c, V x) { VecOps<V>::fma(acc, c, x); }
    static void axis(plx_lattice *L, const double *old, double *out, int a, int vd, const TapArgs64 &taps, hipStream_t stream)
    {
        blur_axis_f64(L, old, out, a, vd, taps, stream);
    }
};

int blur_t_f64_impl(plx_lattice *L, double *d_values, double *d_scratch, int vd, int *result_in_scratch, hipStream_t stream)
{
    return sym_blur_t<double>(L, d_values, d_scratch, vd, result_in_scratch, stream);
}

int blur_sym_f64_planes(const plx_lattice *L) { return sym_planes(L); }

int blur_sym_f64_impl(plx_lattice *L, double *d_values, double *const d_work[3], int vd, double **d_result, hipStream_t stream)
{
    return sym_blur<double>(L, d_values, d_work, vd, d_result, stream);
}

}  // namespace plx
