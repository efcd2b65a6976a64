// plx_query_adjoint.hip -- the splat at query points, S*^T g: the adjoint of plx_slice_at without its 1 / (1 + 2^-d)
// (plx_query_plan / plx_splat_at / plx_splat_at_f64, include/plx.h; the entry points and their argument checks are in
// plx_api.hip).
//
//   values[v] = sum over the corners (r, q) of the located query with vid[r][q] == v of w[r][q] * g[q]
//
// Two steps.  The PLAN, once per located query: the P = nq (d + 1) corner pairs, pair index r * nq + q as they lie in
// memory, sorted by vertex with the build's stable radix sort (plx_sort.hip); an absent corner (id -1) and an id outside
// [0, m) get the key m, so they sort behind every vertex and index nothing.  From the sorted pairs: row[j] = pair % nq,
// w[j] = d_w[pair], and ptr[u] = the first sorted position whose key is >= u, u = 0..m -- the tables of a row range
// (plx_rows.hip), with the queries as the rows; ptr[m] is the number of corners found.  Inside a vertex the corners stand
// in ascending pair index (the sort is stable): that IS the summation order, so two plans of one query give the same bits.
// The SPLAT, one launch of the row-range splat's own kernels over those tables (splat_rows_launch<T>,
// plx_rows_kernels.h): every vertex row is written by exactly one thread per chunk, zeros where no query corner lands,
// no atomics, no zero-fill pass.
//
// Everything lives in the caller's plan buffer, laid out by plan_layout from (m, d, nq) alone; no buffer of the lattice is
// touched, nothing is allocated or read back: launches only, legal under stream capture.
//
// Kernels (256-thread workgroups): query_plan_keys_kernel, the sort's three per pass, query_plan_fill_kernel, rows_ptr_kernel.

#include "plx_kernels.h"

namespace plx {

// ---- the plan buffer -----------------------------------------------------------------------------------------------------
struct PlanLayout {
    size_t ptr, row, w, keys_a, keys_b, vals_a, vals_b, temp, bytes;   // byte offsets of the sections; the whole size
};

static PlanLayout plan_layout(int64_t m, int d, int64_t nq)
{
    const size_t P = (size_t)nq * (d + 1);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    PlanLayout o;
    o.ptr = 0;
    o.row = o.ptr + up(((size_t)m + 1) * 4);
    o.w = o.row + up(P * 4);
    o.keys_a = o.w + up(P * 4);
    o.keys_b = o.keys_a + up(P * 4);
    o.vals_a = o.keys_b + up(P * 4);
    o.vals_b = o.vals_a + up(P * 4);
    o.temp = o.vals_b + up(P * 4);
    o.bytes = o.temp + up(radix_temp_bytes((int64_t)P));
    return o;
}

int64_t query_plan_bytes(int64_t m, int d, int64_t nq) { return (int64_t)plan_layout(m, d, nq).bytes; }

// keys[i] = the vertex of corner pair i, or m where the corner is absent or its id is no vertex of this build
__global__ __launch_bounds__(kBlock) void query_plan_keys_kernel(const int32_t *__restrict__ vid, int P, int m,
                                                                 uint32_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    const uint32_t v = (uint32_t)vid[i];              // a negative id is a large unsigned one
    keys[i] = v < (uint32_t)m ? v : (uint32_t)m;
}

// the sorted pair indices -> the query (row) and the weight of every sorted corner
__global__ __launch_bounds__(kBlock) void query_plan_fill_kernel(const uint32_t *__restrict__ pairs, const float *__restrict__ d_w,
                                                                 int P, int nq, int *__restrict__ row, float *__restrict__ w)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    const uint32_t pair = pairs[j];
    row[j] = (int)(pair % (uint32_t)nq);
    w[j] = d_w[pair];
}

int query_plan_impl(plx_lattice *L, const int32_t *d_vid, const float *d_w, int64_t nq, void *d_plan, hipStream_t stream)
{
    const int m = (int)L->m, P = (int)(nq * (L->d + 1));
    const PlanLayout o = plan_layout(m, L->d, nq);
    char *base = static_cast<char *>(d_plan);
    uint32_t *keys_a = reinterpret_cast<uint32_t *>(base + o.keys_a), *keys_b = reinterpret_cast<uint32_t *>(base + o.keys_b);
    uint32_t *vals_a = reinterpret_cast<uint32_t *>(base + o.vals_a), *vals_b = reinterpret_cast<uint32_t *>(base + o.vals_b);
    const int grid = ceil_div(P, kBlock);
    query_plan_keys_kernel<<<grid, kBlock, 0, stream>>>(d_vid, P, m, keys_a);
    // the key m itself has to be representable (ensure_csr sorts ids up to m - 1: one bit fewer when m is a power of two)
    int end_bit = 1;
    while ((1ll << end_bit) <= (int64_t)m) ++end_bit;
    // first_keys = keys_a: the first pass reads it and writes keys_b, the values 0, 1, 2, ... implied; the second pass is the
    // first to write keys_a
    int second = 0;
    PLX_TRY(radix_sort_pairs32(base + o.temp, keys_a, keys_b, vals_a, vals_b, P, end_bit, &second, stream, keys_a));
    query_plan_fill_kernel<<<grid, kBlock, 0, stream>>>(second ? vals_b : vals_a, d_w, P, (int)nq,
                                                         reinterpret_cast<int *>(base + o.row),
                                                         reinterpret_cast<float *>(base + o.w));
    rows_ptr_launch(reinterpret_cast<const int *>(second ? keys_b : keys_a), P, m, reinterpret_cast<int *>(base + o.ptr), stream);
    PLX_HIP_TRY(hipGetLastError());
    L->kn_plan = "query_plan_keys_kernel+count_kernel+scan_rows_kernel+scatter_kernel+query_plan_fill_kernel+rows_ptr_kernel";
    return PLX_OK;
}

template <typename T>
int splat_at_impl(plx_lattice *L, const void *d_plan, const T *d_g, int vd, int64_t nq, T *d_values, hipStream_t stream)
{
    const PlanLayout o = plan_layout(L->m, L->d, nq);
    const char *base = static_cast<const char *>(d_plan);
    const int *ptr = reinterpret_cast<const int *>(base + o.ptr), *row = reinterpret_cast<const int *>(base + o.row);
    const float *w = reinterpret_cast<const float *>(base + o.w);
    L->kn_splat_at = splat_rows_launch<T>(ptr, row, w, d_g, vd, (int)L->m, d_values, stream);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template int splat_at_impl<float>(plx_lattice *, const void *, const float *, int, int64_t, float *, hipStream_t);
template int splat_at_impl<double>(plx_lattice *, const void *, const double *, int, int64_t, double *, hipStream_t);

}  // namespace plx
