// plx_lanczos.hip -- the fp32 entry points of the Lanczos step: plx_lanczos_kernels.h with T = float (the kernels, the
// span ladder, the dispatch and the checks are all there).
#include "plx_lanczos_kernels.h"

using namespace plx;

extern "C" int plx_lanczos_max_rows(void) { return kLzMaxRows; }

extern "C" int64_t plx_lanczos_work_floats(int64_t n) { return lz_work_count<float>(n); }

extern "C" int plx_lanczos_step(float *d_q, int64_t ld, float *d_w, int64_t n, int i, float *d_alphas, float *d_betas,
                                float *d_work, void *stream)
{
    return lz_step<float>(d_q, ld, d_w, n, i, d_alphas, d_betas, d_work, stream);
}
