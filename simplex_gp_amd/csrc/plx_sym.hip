// plx_sym.hip -- the transposed and the symmetrised fp32 blur on a built lattice (plx_blur_t / plx_blur_sym and the
// products around them): plx_sym_kernels.h with T = float.  The kernel and the launch side are there; here is what fp32
// does in its own way.

#include "plx_sym_kernels.h"

namespace plx {

template <> struct Sym<float> {
    using V1 = float;
    using VN = float4;
    using Taps = TapArgs;
    using Index = uint32_t;      // of a gather; the entry points check m * stride < 2^31
    using Rowlen = uint32_t;
    static constexpr int kPack = 4;
    static int stride(int vd) { return values_stride(vd); }
    // blur_axis_kernel's term: a rounded product, then a rounded sum
    template <class V> static __device__ __forceinline__ void term(V &acc, float c, V x)
    {
        acc = VecOps<V>::add(acc, VecOps<V>::scale(c, x));
    }
    static void axis(plx_lattice *L, const float *cur, float *nxt, int a, int vd, const TapArgs &taps, hipStream_t stream)
    {
        blur_axis_general(L, cur, nxt, a, vd, taps, stream);
    }
};

int blur_t_impl(plx_lattice *L, float *d_values, float *d_scratch, int vd, int *result_in_scratch, hipStream_t stream)
{
    return sym_blur_t<float>(L, d_values, d_scratch, vd, result_in_scratch, stream);
}

int blur_sym_planes(const plx_lattice *L) { return sym_planes(L); }

int blur_sym_impl(plx_lattice *L, float *d_values, float *const d_work[3], int vd, float **d_result, hipStream_t stream)
{
    return sym_blur<float>(L, d_values, d_work, vd, d_result, stream);
}

}  // namespace plx
