// plx_query_f64.hip -- the slice of a float64 vertex array at located queries (plx_slice_at_f64, include/plx.h) and the
// corner dots of its position gradient (plx_slice_at_dots_f64):
// plx_query_kernels.h with T = double.  The sums, the kernels and the launch side are there.

#include "plx_query_kernels.h"

namespace plx {

template int slice_at_impl<double>(plx_lattice *, const double *, int, const int32_t *, const float *, int64_t, double *,
                                   hipStream_t);
template int slice_at_dots_impl<double>(plx_lattice *, const double *, int, const int32_t *, const double *, int64_t, double *,
                                        hipStream_t);

}  // namespace plx
