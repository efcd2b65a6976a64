// plx_rows_f64.hip -- the float64 rectangular product K[out rows, src rows] v: the fp64 splat and slice restricted to a range
// of the caller's rows (plx_splat_rows_f64 / plx_slice_rows_f64 / plx_apply_rows_f64, include/plx.h): plx_rows_kernels.h with
// T = double.  The kernels and the launch side are there; here are the names float64 reports.  The tables are those of
// plx_rows.hip (RowsRange: ptr / row / w per vertex, pos / prow per point): they hold no values, so a range that an fp32 call
// built serves the fp64 call and the reverse.

#include "plx_rows_kernels.h"

namespace plx {

template <> struct Rows<double> {
    static constexpr const char *plx_lattice::*kSplatField = &plx_lattice::kn_rows64_splat;
    static constexpr const char *plx_lattice::*kSliceField = &plx_lattice::kn_rows64_slice;
    static constexpr const char *kSplatV1 = "rows64_splat_v1_kernel";
    static constexpr const char *kSplatChunk = "rows64_splat_chunk_kernel";
    static constexpr const char *kSplatWide = "rows64_splat_wide_kernel";
    static constexpr const char *kSliceV1 = "rows64_slice_v1_kernel";
    static constexpr const char *kSliceChunk = "rows64_slice_chunk_kernel";
    static constexpr const char *kSliceWide = "rows64_slice_wide_kernel";
};

template const char *splat_rows_launch<double>(const int *, const int *, const float *, const double *, int, int, double *,
                                               hipStream_t);
template int splat_rows_impl<double>(plx_lattice *, const double *, int64_t, int64_t, int, double *, hipStream_t);
template int slice_rows_impl<double>(plx_lattice *, const double *, int, int64_t, int64_t, double *, hipStream_t);

}  // namespace plx
