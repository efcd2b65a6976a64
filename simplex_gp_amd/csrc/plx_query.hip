// plx_query.hip -- the slice of an fp32 vertex array at located queries (plx_slice_at, include/plx.h) and the corner
// dots of its position gradient (plx_slice_at_dots):
// plx_query_kernels.h with T = float.  The sums, the kernels and the launch side are there.

#include "plx_query_kernels.h"

namespace plx {

template int slice_at_impl<float>(plx_lattice *, const float *, int, const int32_t *, const float *, int64_t, float *, hipStream_t);
template int slice_at_dots_impl<float>(plx_lattice *, const float *, int, const int32_t *, const float *, int64_t, float *,
                                       hipStream_t);

}  // namespace plx
