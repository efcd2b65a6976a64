// plx_diag_f64.hip -- the true diagonal of the lattice operator in float64 (plx_diag_f64, include/plx.h):
// plx_diag_kernels.h with T = double (the fp32 weights and taps converted exactly).  The identity, the kernel and the
// launch side are there.

#include "plx_diag_kernels.h"

namespace plx {

template int diag_impl<double>(plx_lattice *, int64_t, int64_t, bool, double *, hipStream_t);

}  // namespace plx
