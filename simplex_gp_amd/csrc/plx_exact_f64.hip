// plx_exact_f64.hip -- the float64 entry points of the exact kernel MVM and its position gradient: plx_exact_kernels.h
// with T = double (the kernels, the split rule, the ladders, the dispatch and the checks are all there).
#include "plx_exact_kernels.h"

using namespace plx;

extern "C" int64_t plx_exact_work_bytes_f64(int64_t n1, int64_t n2, int d, int t) { return ex_work_bytes<double>(n1, n2, d, t); }

extern "C" int plx_exact_splits_f64(int64_t n1, int64_t n2, int d, int t) { return ex_splits<double>(n1, n2, d, t); }

extern "C" int plx_exact_mvm_f64(const double *d_x1, int64_t n1, const double *d_x2, int64_t n2, int d, int profile,
                                 const double *d_v, int t, double *d_out, void *d_work, int64_t work_bytes, void *stream)
{
    return ex_run<double>("plx_exact_mvm_f64", false, d_x1, n1, d_x2, n2, d, profile, nullptr, d_v, t, d_out, d_work, work_bytes,
                          stream);
}

extern "C" int plx_exact_grad_f64(const double *d_x1, int64_t n1, const double *d_x2, int64_t n2, int d, int profile,
                                  const double *d_g, const double *d_v, int t, double *d_grad_x1, void *d_work,
                                  int64_t work_bytes, void *stream)
{
    return ex_run<double>("plx_exact_grad_f64", true, d_x1, n1, d_x2, n2, d, profile, d_g, d_v, t, d_grad_x1, d_work, work_bytes,
                          stream);
}
