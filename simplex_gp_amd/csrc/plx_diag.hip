// plx_diag.hip -- the true diagonal of the lattice operator in fp32 (plx_diag, include/plx.h): plx_diag_kernels.h with
// T = float.  The identity, the kernel and the launch side are there.

#include "plx_diag_kernels.h"

namespace plx {

template int diag_impl<float>(plx_lattice *, int64_t, int64_t, bool, float *, hipStream_t);

}  // namespace plx
