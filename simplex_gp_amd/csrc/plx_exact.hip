// plx_exact.hip -- the fp32 entry points of the exact kernel MVM and its position gradient: plx_exact_kernels.h with
// T = float (the kernels, the split rule, the ladders, the dispatch and the checks are all there).
#include "plx_exact_kernels.h"

using namespace plx;

extern "C" int64_t plx_exact_work_bytes(int64_t n1, int64_t n2, int d, int t) { return ex_work_bytes<float>(n1, n2, d, t); }

extern "C" int plx_exact_splits(int64_t n1, int64_t n2, int d, int t) { return ex_splits<float>(n1, n2, d, t); }

extern "C" int plx_exact_mvm(const float *d_x1, int64_t n1, const float *d_x2, int64_t n2, int d, int profile, const float *d_v,
                             int t, float *d_out, void *d_work, int64_t work_bytes, void *stream)
{
    return ex_run<float>("plx_exact_mvm", false, d_x1, n1, d_x2, n2, d, profile, nullptr, d_v, t, d_out, d_work, work_bytes, stream);
}

extern "C" int plx_exact_grad(const float *d_x1, int64_t n1, const float *d_x2, int64_t n2, int d, int profile, const float *d_g,
                              const float *d_v, int t, float *d_grad_x1, void *d_work, int64_t work_bytes, void *stream)
{
    return ex_run<float>("plx_exact_grad", true, d_x1, n1, d_x2, n2, d, profile, d_g, d_v, t, d_grad_x1, d_work, work_bytes, stream);
}
