// plx_rows.hip -- the rectangular product K[out rows, src rows] v: splat and slice restricted to a range of the caller's
// rows (plx_splat_rows / plx_slice_rows / plx_apply_rows, include/plx.h; the entry points and their argument checks are in
// plx_api.hip).  Here: the tables of a row range, which have no scalar type and serve both precisions, and the fp32
// product, plx_rows_kernels.h with T = float -- the splat and slice kernels and their launch side are there.
//
// Per range [begin, begin + count) of caller rows the lattice keeps (RowsRange, plx_internal.h), built by the first call
// that needs them and dropped by the next build:
//   splat side  the corners of those rows in vertex order -- a STABLE compaction of ensure_csr's vertex-sorted arrays
//               (csr_row / csr_w / csr_vid), so the order inside a vertex row is the square splat's and nothing is sorted
//               again -- as (row - begin, weight) pairs plus ptr[m + 1], the first corner of every vertex;
//   slice side  the lattice positions of those rows, ascending (a stable compaction of the point permutation), each with
//               its row - begin.
// Both sizes are known on the host (count (d + 1) and count), so building them reads nothing back.

#include "plx_rows_kernels.h"

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

// ---- the fp32 product: plx_rows_kernels.h with T = float -----------------------------------------------------------
template <> struct Rows<float> {
    static constexpr const char *plx_lattice::*kSplatField = &plx_lattice::kn_rows_splat;
    static constexpr const char *plx_lattice::*kSliceField = &plx_lattice::kn_rows_slice;
    static constexpr const char *kSplatV1 = "rows_splat_v1_kernel";
    static constexpr const char *kSplatChunk = "rows_splat_chunk_kernel";
    static constexpr const char *kSplatWide = "rows_splat_wide_kernel";
    static constexpr const char *kSliceV1 = "rows_slice_v1_kernel";
    static constexpr const char *kSliceChunk = "rows_slice_chunk_kernel";
    static constexpr const char *kSliceWide = "rows_slice_wide_kernel";
};

template const char *splat_rows_launch<float>(const int *, const int *, const float *, const float *, int, int, float *, hipStream_t);
template int splat_rows_impl<float>(plx_lattice *, const float *, int64_t, int64_t, int, float *, hipStream_t);
template int slice_rows_impl<float>(plx_lattice *, const float *, int, int64_t, int64_t, float *, hipStream_t);

}  // namespace plx
