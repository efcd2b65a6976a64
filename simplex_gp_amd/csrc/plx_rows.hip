// plx_rows.hip -- the rectangular product K[out rows, src rows] v: splat and slice restricted to a range of the caller's
// rows (plx_splat_rows / plx_slice_rows / plx_apply_rows, include/plx.h; the entry points and their argument checks are in
// plx_api.hip).  The blur in the middle is plx_blur's.
//
// Per range [begin, begin + count) of caller rows the lattice keeps (RowsRange, plx_internal.h), built by the first call
// that needs them and dropped by the next build:
//   splat side  the corners of those rows in vertex order -- a STABLE compaction of ensure_csr's vertex-sorted arrays
//               (csr_row / csr_w / csr_vid), so the order inside a vertex row is the square splat's and nothing is sorted
//               again -- as (row - begin, weight) pairs plus ptr[m + 1], the first corner of every vertex;
//   slice side  the lattice positions of those rows, ascending (a stable compaction of the point permutation), each with
//               its row - begin.
// Both sizes are known on the host (count (d + 1) and count), so building them reads nothing back.
//
// Kernels (256-thread workgroups, wave64; value rows are whole 16-byte chunks, plx_kernels.h):
//   rows_splat_v1_kernel     vd = 1: one thread per vertex adds up its corners, in order;
//   rows_splat_chunk_kernel  1..64 chunks per row: a group of G = 2^k >= chunks lanes per vertex, one lane per chunk;
//   rows_splat_wide_kernel   more than 64 chunks: one wave per vertex, its lanes stride over the chunks;
//   rows_slice_v1_kernel / rows_slice_chunk_kernel / rows_slice_wide_kernel: the same three shapes per output point.
// Every vertex row is written by exactly one thread per chunk (zero where the range has no corner there): no atomics, no
// zero-fill pass, bitwise reproducible.  Why the gates sit at 1 and 64 chunks: DESIGN.md section 13.

#include "plx_kernels.h"

namespace plx {

// ---- tables: stable compaction by row range ------------------------------------------------------------------------
constexpr int kRowsItems = 8;                       // consecutive entries per thread (order is kept)
constexpr int kRowsTile = kBlock * kRowsItems;

// exclusive scan of one int per thread over the workgroup; *total = the sum
__device__ __forceinline__ int rows_block_scan(int v, int *s, int *total)
{
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int x = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[kBlock - 1];
    __syncthreads();
    return incl - v;
}

// cnt[b] = entries of tile b whose row (keys[i] & mask) lies in [begin, begin + count)
__global__ __launch_bounds__(kBlock) void rows_count_kernel(const uint32_t *__restrict__ keys, uint32_t mask, int total,
                                                            uint32_t begin, uint32_t count, int *__restrict__ cnt)
{
    __shared__ int s[kBlock];
    const int64_t base = (int64_t)blockIdx.x * kRowsTile + (int64_t)threadIdx.x * kRowsItems;
    int c = 0;
    for (int k = 0; k < kRowsItems; ++k) {
        const int64_t i = base + k;
        if (i < total && ((keys[i] & mask) - begin) < count) ++c;
    }
    int sum;
    (void)rows_block_scan(c, s, &sum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = sum;
}

// cnt[0 .. nb) -> exclusive offsets, one workgroup
__global__ __launch_bounds__(kBlock) void rows_offsets_kernel(int *__restrict__ cnt, int nb)
{
    __shared__ int s[kBlock];
    int carry = 0;
    for (int base = 0; base < nb; base += kBlock) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? cnt[i] : 0;
        int sum;
        const int ex = rows_block_scan(v, s, &sum);
        if (i < nb) cnt[i] = carry + ex;
        carry += sum;
    }
}

// CSR = true:  out_a = row - begin, out_w = weight, out_b = vertex of every kept corner (keys = csr_row, head flag masked);
// CSR = false: out_a = row - begin, out_b = lattice position of every kept point (keys = the point permutation)
template <bool CSR>
__global__ __launch_bounds__(kBlock) void rows_compact_kernel(const uint32_t *__restrict__ keys, uint32_t mask, int total,
                                                              uint32_t begin, uint32_t count, const int *__restrict__ off,
                                                              const float *__restrict__ w, const int *__restrict__ vid,
                                                              int kept, int *__restrict__ out_a, float *__restrict__ out_w,
                                                              int *__restrict__ out_b)
{
    __shared__ int s[kBlock];
    const int64_t base = (int64_t)blockIdx.x * kRowsTile + (int64_t)threadIdx.x * kRowsItems;
    uint32_t rel[kRowsItems];
    int c = 0;
    for (int k = 0; k < kRowsItems; ++k) {
        const int64_t i = base + k;
        rel[k] = i < total ? (keys[i] & mask) - begin : 0xFFFFFFFFu;
        if (rel[k] < count) ++c;
    }
    int sum;
    int j = off[blockIdx.x] + rows_block_scan(c, s, &sum);
    for (int k = 0; k < kRowsItems; ++k) {
        if (rel[k] >= count) continue;
        if (j < kept) {                    // (always: the host sized the outputs from the same count)
            const int64_t i = base + k;
            out_a[j] = (int)rel[k];
            if constexpr (CSR) { out_w[j] = w[i]; out_b[j] = vid[i]; }
            else out_b[j] = (int)i;
        }
        ++j;
    }
}

// ptr[u] = first corner whose vertex is >= u, u = 0..m
__global__ __launch_bounds__(kBlock) void rows_ptr_kernel(const int *__restrict__ vid, int kept, int m, int *__restrict__ ptr)
{
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u > m) return;
    int lo = 0, hi = kept;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (vid[mid] < u) lo = mid + 1; else hi = mid;
    }
    ptr[u] = lo;
}

void rows_ptr_launch(const int *vid, int kept, int m, int *ptr, hipStream_t stream)
{
    rows_ptr_kernel<<<ceil_div((int64_t)m + 1, kBlock), kBlock, 0, stream>>>(vid, kept, m, ptr);
}

static int compact_range(plx_lattice *L, const uint32_t *keys, uint32_t mask, int total, int64_t begin, int64_t count,
                         bool csr, int kept, int *out_a, float *out_w, int *out_b, hipStream_t stream)
{
    const int nb = ceil_div(total, kRowsTile);
    PLX_TRY(ensure(L->rows_cnt, (size_t)nb * 4));
    int *cnt = L->rows_cnt.as<int>();
    rows_count_kernel<<<nb, kBlock, 0, stream>>>(keys, mask, total, (uint32_t)begin, (uint32_t)count, cnt);
    rows_offsets_kernel<<<1, kBlock, 0, stream>>>(cnt, nb);
    if (csr)
        rows_compact_kernel<true><<<nb, kBlock, 0, stream>>>(keys, mask, total, (uint32_t)begin, (uint32_t)count, cnt,
                                                             L->csr_w.as<float>(), L->csr_vid.as<int>(), kept, out_a, out_w,
                                                             out_b);
    else
        rows_compact_kernel<false><<<nb, kBlock, 0, stream>>>(keys, mask, total, (uint32_t)begin, (uint32_t)count, cnt,
                                                              nullptr, nullptr, kept, out_a, nullptr, out_b);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

// The slot of a range: the one that holds it, else an empty one, else the least recently used.
plx_lattice::RowsRange *range_slot(plx_lattice *L, int64_t begin, int64_t count)
{
    plx_lattice::RowsRange *pick = nullptr;
    for (auto &r : L->rows) {
        if (r.gen == L->build_gen && r.begin == begin && r.count == count) { pick = &r; break; }
    }
    if (!pick) {
        for (auto &r : L->rows) {
            if (r.gen != L->build_gen) { pick = &r; break; }          // empty, or of an earlier build
            if (!pick || r.used < pick->used) pick = &r;
        }
        pick->gen = L->build_gen;
        pick->begin = begin;
        pick->count = count;
        pick->splat_ready = pick->slice_ready = false;
    }
    pick->used = ++L->rows_clock;
    return pick;
}

int ensure_rows_splat(plx_lattice *L, plx_lattice::RowsRange *r, hipStream_t stream)
{
    if (r->splat_ready) return PLX_OK;
    PLX_TRY(refuse_under_capture(stream, "the corner table of this row range"));
    PLX_TRY(ensure_csr(L, stream));
    const int kept = (int)(r->count * (L->d + 1)), m = (int)L->m;
    PLX_TRY(ensure(r->row, (size_t)kept * 4));
    PLX_TRY(ensure(r->w, (size_t)kept * 4));
    PLX_TRY(ensure(r->ptr, (size_t)(m + 1) * 4));
    PLX_TRY(ensure(L->rows_vid, (size_t)kept * 4));
    PLX_TRY(compact_range(L, L->csr_row.as<uint32_t>(), 0x7FFFFFFFu, (int)L->nnz, r->begin, r->count, true, kept,
                          r->row.as<int>(), r->w.as<float>(), L->rows_vid.as<int>(), stream));
    rows_ptr_launch(L->rows_vid.as<int>(), kept, m, r->ptr.as<int>(), stream);
    PLX_HIP_TRY(hipGetLastError());
    r->splat_ready = true;
    return PLX_OK;
}

int ensure_rows_slice(plx_lattice *L, plx_lattice::RowsRange *r, hipStream_t stream)
{
    if (r->slice_ready) return PLX_OK;
    PLX_TRY(refuse_under_capture(stream, "the position table of this row range"));
    PLX_TRY(ensure(r->pos, (size_t)r->count * 4));
    PLX_TRY(ensure(r->prow, (size_t)r->count * 4));
    PLX_TRY(compact_range(L, L->perm.as<uint32_t>(), 0xFFFFFFFFu, (int)L->n, r->begin, r->count, false, (int)r->count,
                          r->prow.as<int>(), nullptr, r->pos.as<int>(), stream));
    r->slice_ready = true;
    return PLX_OK;
}

// ---- splat ---------------------------------------------------------------------------------------------------------
// one chunk of a source row: a 16-byte load where the rows are whole aligned chunks, else per float with the tail guarded
template <bool VEC>
__device__ __forceinline__ float4 rows_load_chunk(const float *__restrict__ src, size_t row, int vd, int ch)
{
    const float *p = src + row * vd + 4 * ch;
    if constexpr (VEC) return *reinterpret_cast<const float4 *>(p);
    const int left = vd - 4 * ch;
    float4 x = f4_zero();
    x.x = p[0];
    if (left > 1) x.y = p[1];
    if (left > 2) x.z = p[2];
    if (left > 3) x.w = p[3];
    return x;
}

template <bool VEC>
__device__ __forceinline__ void rows_store_chunk(float *__restrict__ out, size_t row, int vd, int ch, float4 a)
{
    float *o = out + row * vd + 4 * ch;
    if constexpr (VEC) { *reinterpret_cast<float4 *>(o) = a; return; }
    const int left = vd - 4 * ch;
    o[0] = a.x;
    if (left > 1) o[1] = a.y;
    if (left > 2) o[2] = a.z;
    if (left > 3) o[3] = a.w;
}

template <bool VEC>
__device__ __forceinline__ float4 rows_vertex_sum(const int *__restrict__ row, const float *__restrict__ w, int j0, int j1,
                                                  const float *__restrict__ src, int vd, int ch)
{
    float4 acc = f4_zero();
    for (int j = j0; j < j1; ++j) {
        const float wj = w[j];
        const float4 x = rows_load_chunk<VEC>(src, (size_t)row[j], vd, ch);
        acc.x += wj * x.x; acc.y += wj * x.y; acc.z += wj * x.z; acc.w += wj * x.w;
    }
    return acc;
}

__global__ __launch_bounds__(kBlock) void rows_splat_v1_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                               const float *__restrict__ w, const float *__restrict__ src,
                                                               int m, float *__restrict__ values)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    float acc = 0.f;
    for (int j = ptr[v], j1 = ptr[v + 1]; j < j1; ++j) acc += w[j] * src[row[j]];
    values[v] = acc;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void rows_splat_chunk_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                  const float *__restrict__ w, const float *__restrict__ src,
                                                                  int vd, int nch, int shift, int m,
                                                                  float4 *__restrict__ values)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (v >= m || ch >= nch) return;
    values[(size_t)v * nch + ch] = rows_vertex_sum<VEC>(row, w, ptr[v], ptr[v + 1], src, vd, ch);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void rows_splat_wide_kernel(const int *__restrict__ ptr, const int *__restrict__ row,
                                                                 const float *__restrict__ w, const float *__restrict__ src,
                                                                 int vd, int nch, int m, float4 *__restrict__ values)
{
    const int64_t v = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= m) return;
    const int j0 = ptr[v], j1 = ptr[v + 1];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        values[(size_t)v * nch + ch] = rows_vertex_sum<VEC>(row, w, j0, j1, src, vd, ch);
}

// ---- slice ---------------------------------------------------------------------------------------------------------
// (rows_point_sum and rows_filtered_chunk, the sums of a filtered chunk: plx_kernels.h, shared with the fp32 trait of
// plx_rows_backward_kernels.h in plx_rows_backward.hip)
__global__ __launch_bounds__(kBlock) void rows_slice_v1_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                               const int *__restrict__ evid, const float *__restrict__ ew,
                                                               int n, int d1, int count, const float *__restrict__ values,
                                                               float rden, float *__restrict__ out)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    const int p = pos[j];
    float acc = 0.f;
    for (int r = 0; r < d1; ++r) acc += ew[(size_t)r * n + p] * values[evid[(size_t)r * n + p]] * rden;
    out[prow[j]] = acc;
}

// D1 > 0: d + 1 compiled in (all index / weight loads, then all gathers, then the ordered sum); 0: the run-time form
template <bool VEC, int D1>
__global__ __launch_bounds__(kBlock) void rows_slice_chunk_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                                  const int *__restrict__ evid, const float *__restrict__ ew,
                                                                  int n, int d1, int count,
                                                                  const float4 *__restrict__ values, int vd, int nch,
                                                                  int shift, float rden, float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j = t >> shift;
    const int ch = (int)(t & ((1 << shift) - 1));
    if (j >= count || ch >= nch) return;
    const float4 acc = rows_filtered_chunk<D1>(evid, ew, n, pos[j], d1, values, nch, ch, rden);
    rows_store_chunk<VEC>(out, (size_t)prow[j], vd, ch, acc);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void rows_slice_wide_kernel(const int *__restrict__ pos, const int *__restrict__ prow,
                                                                 const int *__restrict__ evid, const float *__restrict__ ew,
                                                                 int n, int d1, int count, const float4 *__restrict__ values,
                                                                 int vd, int nch, float rden, float *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (j >= count) return;
    const int p = pos[j];
    const size_t row = (size_t)prow[j];
    for (int ch = threadIdx.x & 63; ch < nch; ch += 64)
        rows_store_chunk<VEC>(out, row, vd, ch, rows_point_sum(evid, ew, n, p, d1, values, nch, ch, rden));
}

// ---- launch side ---------------------------------------------------------------------------------------------------
constexpr int kRowsChunkMax = 64;     // chunks one lane group can cover: a group never spans two waves

static inline bool rows_vec_ok(const void *p, int vd) { return (vd & 3) == 0 && ((uintptr_t)p & 15) == 0; }
static inline int rows_group_shift(int nch)
{
    int s = 0;
    while ((1 << s) < nch) ++s;
    return s;
}

const char *splat_rows_launch(const int *ptr, const int *row, const float *w, const float *d_src, int vd, int m, float *d_values,
                              hipStream_t stream)
{
    const int nch = values_stride(vd) / 4;
    const bool vec = rows_vec_ok(d_src, vd);
    float4 *v4 = reinterpret_cast<float4 *>(d_values);
    const char *kn_rows_splat;            // (named as the member the row-range splat keeps it in)
    if (vd == 1) {
        kn_rows_splat = "rows_splat_v1_kernel";
        rows_splat_v1_kernel<<<ceil_div(m, kBlock), kBlock, 0, stream>>>(ptr, row, w, d_src, m, d_values);
    } else if (nch <= kRowsChunkMax) {
        kn_rows_splat = "rows_splat_chunk_kernel";
        const int shift = rows_group_shift(nch);
        const int grid = ceil_div((int64_t)m << shift, kBlock);
        if (vec) rows_splat_chunk_kernel<true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, v4);
        else rows_splat_chunk_kernel<false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, shift, m, v4);
    } else {
        kn_rows_splat = "rows_splat_wide_kernel";
        const int grid = ceil_div(m, kBlock / 64);
        if (vec) rows_splat_wide_kernel<true><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, v4);
        else rows_splat_wide_kernel<false><<<grid, kBlock, 0, stream>>>(ptr, row, w, d_src, vd, nch, m, v4);
    }
    return kn_rows_splat;
}

int splat_rows_impl(plx_lattice *L, const float *d_src, int64_t begin, int64_t count, int vd, float *d_values,
                           hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, begin, count);
    PLX_TRY(ensure_rows_splat(L, r, stream));
    L->kn_rows_splat = splat_rows_launch(r->ptr.as<int>(), r->row.as<int>(), r->w.as<float>(), d_src, vd, (int)L->m, d_values,
                                         stream);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

template <bool VEC>
static void launch_slice_chunk(plx_lattice *L, const plx_lattice::RowsRange *r, const float4 *v4, int vd, int nch, float rden,
                               float *d_out, hipStream_t stream)
{
    const int n = (int)L->n, d1 = L->d + 1, count = (int)r->count;
    const int shift = rows_group_shift(nch);
    const int grid = ceil_div((int64_t)count << shift, kBlock);
    const int *pos = r->pos.as<int>(), *prow = r->prow.as<int>();
    const int *evid = L->evid.as<int>();
    const float *ew = L->ew.as<float>();
    dispatch_d1(d1, [&](auto D1) {
        rows_slice_chunk_kernel<VEC, decltype(D1)::value><<<grid, kBlock, 0, stream>>>(pos, prow, evid, ew, n, d1,
                                                                                       count, v4, vd, nch, shift, rden,
                                                                                       d_out);
    });
}

int slice_rows_impl(plx_lattice *L, const float *d_values, int vd, int64_t begin, int64_t count, float *d_out,
                           hipStream_t stream)
{
    plx_lattice::RowsRange *r = range_slot(L, begin, count);
    PLX_TRY(ensure_rows_slice(L, r, stream));
    const int n = (int)L->n, d1 = L->d + 1, nch = values_stride(vd) / 4;
    const float rden = 1.0f / L->slice_denom;
    const bool vec = rows_vec_ok(d_out, vd);
    const float4 *v4 = reinterpret_cast<const float4 *>(d_values);
    if (vd == 1) {
        L->kn_rows_slice = "rows_slice_v1_kernel";
        rows_slice_v1_kernel<<<ceil_div(count, kBlock), kBlock, 0, stream>>>(r->pos.as<int>(), r->prow.as<int>(),
                                                                              L->evid.as<int>(), L->ew.as<float>(), n, d1,
                                                                              (int)count, d_values, rden, d_out);
    } else if (nch <= kRowsChunkMax) {
        L->kn_rows_slice = "rows_slice_chunk_kernel";
        if (vec) launch_slice_chunk<true>(L, r, v4, vd, nch, rden, d_out, stream);
        else launch_slice_chunk<false>(L, r, v4, vd, nch, rden, d_out, stream);
    } else {
        L->kn_rows_slice = "rows_slice_wide_kernel";
        const int grid = ceil_div(count, kBlock / 64);
        if (vec)
            rows_slice_wide_kernel<true><<<grid, kBlock, 0, stream>>>(r->pos.as<int>(), r->prow.as<int>(), L->evid.as<int>(),
                                                                      L->ew.as<float>(), n, d1, (int)count, v4, vd, nch, rden,
                                                                      d_out);
        else
            rows_slice_wide_kernel<false><<<grid, kBlock, 0, stream>>>(r->pos.as<int>(), r->prow.as<int>(), L->evid.as<int>(),
                                                                       L->ew.as<float>(), n, d1, (int)count, v4, vd, nch, rden,
                                                                       d_out);
    }
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
