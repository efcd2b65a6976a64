// plx_lanczos_f64.hip -- the float64 entry points of the Lanczos step: plx_lanczos_kernels.h with T = double (the
// kernels, the span ladder, the dispatch and the checks are all there).
#include "plx_lanczos_kernels.h"

using namespace plx;

extern "C" int64_t plx_lanczos_work_doubles(int64_t n) { return lz_work_count<double>(n); }

extern "C" int plx_lanczos_shape_f64(int64_t n, int *span, int *groups)
{
    if (lz_work_count<double>(n) < 0) {
        set_error("plx_lanczos_shape_f64: n = %lld outside 1..%lld", (long long)n,
                  (long long)LzScalar<double>::kMaxGroups * kLzMaxSpan<double>);
        return PLX_ERR_INVALID;
    }
    const LzShape sh = lz_shape<double>(n);
    if (span) *span = sh.span;
    if (groups) *groups = sh.groups;
    return PLX_OK;
}

extern "C" int plx_lanczos_step_f64(double *d_q, int64_t ld, double *d_w, int64_t n, int i, double *d_alphas, double *d_betas,
                                    double *d_work, void *stream)
{
    return lz_step<double>(d_q, ld, d_w, n, i, d_alphas, d_betas, d_work, stream);
}
