// plx_api.hip -- extern "C" entry points declared in include/plx.h.
#include "plx_internal.h"

#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace plx {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// The stream of the entry point that is running on this thread: buffers grow stream-ordered on it (hipFreeAsync +
// hipMallocAsync), so the first MVM that needs a wider workspace does not synchronise the device the way hipFree does.
static thread_local hipStream_t g_entry_stream = nullptr;
// ... and the switches of the lattice it serves (Tune): a build takes a fresh snapshot of the process defaults first.
struct EntryScope {
    hipStream_t prev;
    const Tune *prev_tune;
    EntryScope(plx_lattice *L, void *s) : prev(g_entry_stream), prev_tune(tl_tune)
    {
        g_entry_stream = (hipStream_t)s;
        tl_tune = L ? &L->tn : &g_tune_defaults;
    }
    ~EntryScope() { g_entry_stream = prev; tl_tune = prev_tune; }
};

int refuse_under_capture(hipStream_t stream, const char *what)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
        set_error("%s has to be built or grown (an allocation, for tables also a host read-back) and the stream is being "
                  "captured: call plx_prepare(lat, vd, stream) and run one MVM of this width before the capture", what);
        return PLX_ERR_STATE;
    }
    return PLX_OK;
}

int ensure(DevBuf &b, size_t bytes)
{
    if (bytes == 0) bytes = 4;
    if (b.cap >= bytes) return PLX_OK;
    const hipStream_t s = g_entry_stream;
    // growing a buffer inside a capture would hand the lattice an address that belongs to the graph (a captured
    // hipMallocAsync is a memory node: the memory exists while the graph runs, not afterwards)
    PLX_TRY(refuse_under_capture(s, "a device buffer of this lattice"));
    if (b.p) {
        // work queued on another stream may still read the old buffer.  The stored handle is only COMPARED, never used:
        // its owner may have destroyed that stream since (and the runtime may have recycled the handle), so the wait is
        // for the device.  Growth across streams is rare -- a lattice normally lives on one stream.
        if (b.owner != s) PLX_HIP_TRY(hipDeviceSynchronize());
        PLX_HIP_TRY(hipFreeAsync(b.p, s));
        b.p = nullptr;
        b.cap = 0;
    }
    PLX_HIP_TRY(hipMallocAsync(&b.p, bytes, s));
    b.cap = bytes;
    b.owner = s;
    return PLX_OK;
}

void release(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

static std::vector<DevBuf *> all_bufs(plx_lattice *L)
{
    std::vector<DevBuf *> v = {&L->eslot, &L->flagmask, &L->blockcnt, &L->table, &L->counters,
            &L->sort_keys_in, &L->slotmap, &L->nibmap, &L->prank, &L->vaxis, &L->vs0, &L->vowner, &L->ew_splat, &L->replay_vat, &L->replay_list, &L->replay_invisible, &L->replay_keys, &L->active_list, &L->active_cnt, &L->oh_pos, &L->oh_list, &L->oh_cnt, &L->ex_vid, &L->ex_pt, &L->ex_w, &L->ex_keys, &L->sort_vals_in, &L->sort_vals_out, &L->sort_temp,
            &L->vkeys, &L->ew, &L->evid, &L->nbr, &L->csr_pt, &L->csr_row, &L->csr_w, &L->csr_vid, &L->row_ptr,
            &L->head_partial, &L->tail_partial, &L->val_a, &L->val_b, &L->ssrc, &L->rec, &L->perm, &L->iota, &L->cmask, &L->cbase, &L->cids, &L->merge_slot, &L->merge_flags,
            &L->sortkey_in, &L->sortkey_out,
            &L->bc_pt, &L->bc_w, &L->srow, &L->brow_ptr, &L->brow_vid, &L->s2_idx, &L->s2_ptr, &L->s2_vid, &L->s2_wave, &L->s2_wave_v, &L->partial, &L->pair_nbr, &L->inv_perm, &L->vslot, &L->vkeys_alt, &L->vslot_alt, &L->vorder,
            &L->rows_cnt, &L->rows_vid, &L->val64_a, &L->val64_b, &L->val64_s, &L->val_s};
    for (auto &r : L->rows)
        for (DevBuf *b : {&r.ptr, &r.row, &r.w, &r.pos, &r.prow}) v.push_back(b);
    return v;
}

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace plx

using namespace plx;

extern "C" {

const char *plx_strerror(int code)
{
    switch (code) {
    case PLX_OK: return "ok";
    case PLX_ERR_INVALID: return "invalid argument";
    case PLX_ERR_HIP: return "HIP runtime error";
    case PLX_ERR_KEY_RANGE: return "lattice coordinate outside the int16 key range";
    case PLX_ERR_DIM: return "dimension or order outside the compiled range";
    case PLX_ERR_STATE: return "lattice not built or size mismatch";
    case PLX_ERR_TOO_LARGE: return "n*(d+1) exceeds the 31-bit entry index";
    default: return "unknown error";
    }
}

const char *plx_last_error(void) { return g_err; }

/* minor = the round that last extended the C ABI */
const char *plx_version(void) { return "libplx 0.9.1 gfx950"; }

int plx_create(int device, plx_lattice **out)
{
    if (!out) { set_error("plx_create: out is NULL"); return PLX_ERR_INVALID; }
    DeviceGuard g(device);
    if (!g.ok) { set_error("plx_create: cannot select device %d", device); return PLX_ERR_HIP; }
    plx_lattice *L = new plx_lattice();
    L->device = device;
    if (hipHostMalloc((void **)&L->h_pinned, 256, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&L->h_mail, 256, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        set_error("plx_create: hipHostMalloc failed");
        if (L->h_pinned) (void)hipHostFree(L->h_pinned);
        delete L;
        return PLX_ERR_HIP;
    }
    memset(L->h_mail, 0, 256);
    // on failure plx_destroy releases whatever was created so far (events not yet created are null)
    for (auto &e : L->ev)
        if (hipEventCreate(&e) != hipSuccess) { e = nullptr; plx_destroy(L); set_error("plx_create: hipEventCreate failed"); return PLX_ERR_HIP; }
    for (auto &e : L->tev)
        if (hipEventCreate(&e) != hipSuccess) { e = nullptr; plx_destroy(L); set_error("plx_create: hipEventCreate failed"); return PLX_ERR_HIP; }
    *out = L;
    return PLX_OK;
}

void plx_destroy(plx_lattice *L)
{
    if (!L) return;
    DeviceGuard g(L->device);
    for (DevBuf *b : all_bufs(L)) release(*b);
    if (L->h_pinned) (void)hipHostFree(L->h_pinned);
    if (L->h_mail) (void)hipHostFree(L->h_mail);
    for (auto &e : L->ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : L->tev) if (e) (void)hipEventDestroy(e);
    delete L;
}

// single_use: the lattice serves ONE MVM (plx_filter, the reference's one-shot contract): what only pays back over several
// MVMs is left out of the build -- the vertex renumbering (+0.16 ms for -17 us per MVM at N = 1e6), the axis-pair tables
// and, for a multi-column MVM, the block tables.
static int build_entry(plx_lattice *L, const float *d_ref, int64_t n, int d, const float *h_taps, int ntaps,
                       int shard_index, int n_shards, void *stream, bool single_use)
{
    EntryScope sc(L, stream);
    if (!L || !d_ref || !h_taps) { set_error("plx_build: NULL argument"); return PLX_ERR_INVALID; }
    if (n <= 0) { set_error("plx_build: n = %lld must be positive", (long long)n); return PLX_ERR_INVALID; }
    if (d < 1 || d > PLX_MAX_DIM) { set_error("plx_build: d = %d outside 1..%d", d, PLX_MAX_DIM); return PLX_ERR_DIM; }
    if (ntaps < 1 || (ntaps % 2) == 0) { set_error("plx_build: tap count %d must be odd", ntaps); return PLX_ERR_INVALID; }
    if (ntaps / 2 > PLX_MAX_ORDER) { set_error("plx_build: order %d > %d", ntaps / 2, PLX_MAX_ORDER); return PLX_ERR_DIM; }
    if (n_shards < 1 || n_shards > 256 || shard_index < 0 || shard_index >= n_shards) {
        set_error("plx_build: shard %d of %d is not a valid shard (1..256 shards)", shard_index, n_shards);
        return PLX_ERR_INVALID;
    }
    if (n * (int64_t)(d + 1) >= (1ll << 31) - 1024) {
        set_error("plx_build: n*(d+1) = %lld does not fit the 31-bit entry index", (long long)(n * (d + 1)));
        return PLX_ERR_TOO_LARGE;
    }
    DeviceGuard g(L->device);
    if (!g.ok) { set_error("plx_build: cannot select device %d", L->device); return PLX_ERR_HIP; }
    L->tn = g_tune_defaults;       // the snapshot of the process defaults this build (and every later call on it) runs under:
                                   // taken only once the arguments are accepted -- a rejected call leaves a built lattice as it was
    L->built = false;
    L->build_gen++;                // the row-range tables of earlier builds (plx_rows.hip) are stale from here on
    L->local_ready = false;
    L->single_use = single_use;
    L->n = n; L->d = d; L->ntaps = ntaps; L->order = ntaps / 2;
    L->shard_index = shard_index; L->n_shards = n_shards;
    shard_range(n, n_shards, shard_index, &L->own_begin, &L->own_end);
    memset(&L->taps, 0, sizeof(L->taps));
    for (int i = 0; i < ntaps; ++i) L->taps.c[i] = h_taps[i];
    int rc = build_impl(L, d_ref, (hipStream_t)stream);
    if (rc == PLX_OK) L->built = true;
    return rc;
}

int plx_build(plx_lattice *L, const float *d_ref, int64_t n, int d, const float *h_taps, int ntaps,
              int shard_index, int n_shards, void *stream)
{
    return build_entry(L, d_ref, n, d, h_taps, ntaps, shard_index, n_shards, stream, false);
}

// ---- sharded build: local stage, key exchange by the caller, merge stage ------------------------

int plx_build_local(plx_lattice *L, const float *d_ref_local, int64_t n_local, int d, const float *h_taps, int ntaps,
                    void *stream)
{
    EntryScope sc(L, stream);
    if (!L || !d_ref_local || !h_taps) { set_error("plx_build_local: NULL argument"); return PLX_ERR_INVALID; }
    if (n_local <= 0) { set_error("plx_build_local: n_local = %lld must be positive", (long long)n_local); return PLX_ERR_INVALID; }
    if (d < 1 || d > PLX_MAX_DIM) { set_error("plx_build_local: d = %d outside 1..%d", d, PLX_MAX_DIM); return PLX_ERR_DIM; }
    if (ntaps < 1 || (ntaps % 2) == 0) { set_error("plx_build_local: tap count %d must be odd", ntaps); return PLX_ERR_INVALID; }
    if (ntaps / 2 > PLX_MAX_ORDER) { set_error("plx_build_local: order %d > %d", ntaps / 2, PLX_MAX_ORDER); return PLX_ERR_DIM; }
    if (n_local * (int64_t)(d + 1) >= (1ll << 31) - 1024) {
        set_error("plx_build_local: n*(d+1) = %lld does not fit the 31-bit entry index", (long long)(n_local * (d + 1)));
        return PLX_ERR_TOO_LARGE;
    }
    DeviceGuard g(L->device);
    if (!g.ok) { set_error("plx_build_local: cannot select device %d", L->device); return PLX_ERR_HIP; }
    L->tn = g_tune_defaults;
    L->built = false;
    L->build_gen++;
    L->local_ready = false;
    L->n = n_local; L->d = d; L->ntaps = ntaps; L->order = ntaps / 2;
    L->shard_index = 0; L->n_shards = 1;
    L->own_begin = 0; L->own_end = n_local;
    memset(&L->taps, 0, sizeof(L->taps));
    for (int i = 0; i < ntaps; ++i) L->taps.c[i] = h_taps[i];
    L->for_merge = true;
    L->single_use = false;
    int rc = build_local_impl(L, d_ref_local, (hipStream_t)stream);
    L->for_merge = false;
    if (rc == PLX_OK) L->local_ready = true;
    return rc;
}

int plx_key_words(int d) { return (d >= 1 && d <= PLX_MAX_DIM) ? (d + 1) / 2 : -1; }

int64_t plx_local_vertices(const plx_lattice *L) { return (L && (L->local_ready || L->built)) ? L->m : -1; }

int plx_copy_local_keys(plx_lattice *L, void *d_dst, void *stream)
{
    EntryScope sc(L, stream);
    if (!L || !d_dst) { set_error("plx_copy_local_keys: NULL argument"); return PLX_ERR_INVALID; }
    if (!L->local_ready) { set_error("plx_copy_local_keys: call plx_build_local first"); return PLX_ERR_STATE; }
    DeviceGuard g(L->device);
    PLX_HIP_TRY(hipMemcpyAsync(d_dst, L->vkeys.p, (size_t)L->m * plx_key_words(L->d) * 4, hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
    return PLX_OK;
}

int plx_build_merge(plx_lattice *L, const void *d_all_keys, const int64_t *h_counts, int n_ranks, int my_rank, int64_t total_points,
                    void *stream)
{
    EntryScope sc(L, stream);
    if (!L || !d_all_keys || !h_counts) { set_error("plx_build_merge: NULL argument"); return PLX_ERR_INVALID; }
    if (!L->local_ready) { set_error("plx_build_merge: call plx_build_local first"); return PLX_ERR_STATE; }
    if (n_ranks < 1 || my_rank < 0 || my_rank >= n_ranks) {
        set_error("plx_build_merge: rank %d of %d", my_rank, n_ranks);
        return PLX_ERR_INVALID;
    }
    DeviceGuard g(L->device);
    if (!g.ok) { set_error("plx_build_merge: cannot select device %d", L->device); return PLX_ERR_HIP; }
    L->merge_total_points = total_points;
    int rc = build_merge_impl(L, (const uint32_t *)d_all_keys, h_counts, n_ranks, my_rank, (hipStream_t)stream);
    L->local_ready = false;
    if (rc == PLX_OK) L->built = true;
    return rc;
}

int64_t plx_num_points(const plx_lattice *L) { return L ? L->n : -1; }
int64_t plx_num_owned(const plx_lattice *L) { return L ? L->own_end - L->own_begin : -1; }
int64_t plx_num_vertices(const plx_lattice *L) { return (L && L->built) ? L->m : -1; }

int plx_reference_growth_info(const plx_lattice *L, int64_t *h_out6)
{
    if (!L || !L->built || !h_out6) { set_error("plx_reference_growth_info: lattice not built"); return PLX_ERR_STATE; }
    const auto &rp = L->replay;
    h_out6[0] = rp.active ? 1 : 0;
    h_out6[1] = rp.active ? rp.m_reference : L->m;
    h_out6[2] = rp.n_dropped;
    h_out6[3] = rp.n_invisible;
    h_out6[4] = rp.blur_miss ? 1 : 0;
    h_out6[5] = rp.inexact ? 1 : 0;
    return PLX_OK;
}
int plx_dim(const plx_lattice *L) { return L ? L->d : -1; }
int plx_order(const plx_lattice *L) { return L ? L->order : -1; }

int plx_set_row_order(plx_lattice *L, int lattice_order)
{
    if (!L) { set_error("plx_set_row_order: NULL lattice"); return PLX_ERR_INVALID; }
    L->lattice_rows = lattice_order != 0;
    return PLX_OK;
}

int plx_set_reuse_order(plx_lattice *L, int on)
{
    if (!L) { set_error("plx_set_reuse_order: NULL lattice"); return PLX_ERR_INVALID; }
    L->reuse_order = on != 0;
    return PLX_OK;
}

int plx_order_age(const plx_lattice *L) { return L ? (L->order_n > 0 ? L->order_age : -1) : -1; }

int plx_values_stride(int vd) { return vd >= 1 ? values_stride(vd) : -1; }

int64_t plx_device_bytes(const plx_lattice *L)
{
    if (!L) return -1;
    int64_t total = 0;
    for (DevBuf *b : all_bufs(const_cast<plx_lattice *>(L))) total += (int64_t)b->cap;
    return total;
}

// What every product call checks first: its arguments, a built lattice, a positive width.
static int check_call(const plx_lattice *L, const void *a, const void *b, int vd, const char *who)
{
    if (!L || !a || !b) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (!L->built) { set_error("%s: lattice not built", who); return PLX_ERR_STATE; }
    if (vd < 1) { set_error("%s: vd = %d must be positive", who, vd); return PLX_ERR_INVALID; }
    return PLX_OK;
}

// The row-range and float64 products run on plain single-shard builds only.  `what`: the product with its verb, "row
// ranges are" or "the float64 product is", as in
//   "plx_apply_rows (source rows): sharded or merged lattice (row ranges are served by plain single-shard builds only)"
//   "plx_apply_f64: this build replayed "reference_growth" (its splat and slice sides differ); the float64 product is
//    not served on it"
static int check_plain_build(const plx_lattice *L, const char *what, const char *who)
{
    if (L->n_shards != 1 || L->partial_cover) {
        set_error("%s: sharded or merged lattice (%s served by plain single-shard builds only)", who, what);
        return PLX_ERR_STATE;
    }
    if (L->replay.active) {
        set_error("%s: this build replayed \"reference_growth\" (its splat and slice sides differ); %s not served on it", who,
                  what);
        return PLX_ERR_STATE;
    }
    return PLX_OK;
}

static int check_apply(const plx_lattice *L, const void *a, const void *b, int vd, const char *who)
{
    PLX_TRY(check_call(L, a, b, vd, who));
    if ((int64_t)L->m * values_stride(vd) >= (1ll << 31) ||
        (int64_t)(L->own_end - L->own_begin) * values_stride(vd) >= (1ll << 31)) {
        set_error("%s: m*vd or n*vd exceeds 2^31 elements; split the columns", who);
        return PLX_ERR_TOO_LARGE;
    }
    return PLX_OK;
}

int plx_splat(plx_lattice *L, const float *d_src, int vd, float *d_values, void *stream)
{
    EntryScope sc(L, stream);
    // a rank that owns no rows has no source block: only the accumulator is required
    if (L && L->built && L->own_end == L->own_begin && !d_src) d_src = d_values;
    PLX_TRY(check_apply(L, d_src, d_values, vd, "plx_splat"));
    DeviceGuard g(L->device);
    return splat_impl(L, d_src, vd, d_values, (hipStream_t)stream);
}

int plx_splat_onehot(plx_lattice *L, const int32_t *d_points, int nb, int vd, float *d_values, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_apply(L, d_points, d_values, vd, "plx_splat_onehot"));
    if (nb < 1 || nb > vd) { set_error("plx_splat_onehot: %d one-hot columns in %d", nb, vd); return PLX_ERR_INVALID; }
    if (L->n_shards != 1 || L->partial_cover) { set_error("plx_splat_onehot: single-shard lattices only"); return PLX_ERR_STATE; }
    DeviceGuard g(L->device);
    return splat_onehot_impl(L, d_points, nb, vd, d_values, (hipStream_t)stream);
}

int plx_filter_onehot(plx_lattice *L, const int32_t *d_points, int nb, int vd, float *d_values, float *d_scratch, float *d_out,
                      int sparse, int32_t *d_frontier, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_apply(L, d_values, d_scratch, vd, "plx_filter_onehot"));
    if (!d_points || !d_out) { set_error("plx_filter_onehot: NULL argument"); return PLX_ERR_INVALID; }
    if (d_values == d_scratch) { set_error("plx_filter_onehot: d_values and d_scratch must be different buffers"); return PLX_ERR_INVALID; }
    if (nb < 1 || nb > vd || nb > 16) { set_error("plx_filter_onehot: %d one-hot columns in %d (at most 16)", nb, vd); return PLX_ERR_INVALID; }
    if (L->n_shards != 1 || L->partial_cover) { set_error("plx_filter_onehot: single-shard lattices only"); return PLX_ERR_STATE; }
    DeviceGuard g(L->device);
    return filter_onehot_impl(L, d_points, nb, vd, d_values, d_scratch, d_out, sparse, d_frontier, (hipStream_t)stream);
}

int plx_blur(plx_lattice *L, float *d_values, float *d_scratch, int vd, int *result_in_scratch, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_apply(L, d_values, d_scratch, vd, "plx_blur"));
    if (!result_in_scratch) { set_error("plx_blur: result_in_scratch is NULL"); return PLX_ERR_INVALID; }
    DeviceGuard g(L->device);
    return blur_impl(L, d_values, d_scratch, vd, result_in_scratch, (hipStream_t)stream);
}

int plx_slice(plx_lattice *L, const float *d_values, int vd, float *d_out, void *stream)
{
    EntryScope sc(L, stream);
    if (L && L->built && L->own_end == L->own_begin && !d_out) d_out = const_cast<float *>(d_values);
    PLX_TRY(check_apply(L, d_values, d_out, vd, "plx_slice"));
    DeviceGuard g(L->device);
    return slice_impl(L, d_values, vd, d_out, (hipStream_t)stream);
}

static int apply_common(plx_lattice *L, const float *d_src, int vd, float *d_out, const float *d_affine, void *stream,
                        const char *who);

int plx_apply_affine(plx_lattice *L, const float *d_src, int vd, float *d_out, const float *d_scale_shift, void *stream)
{
    if (!d_scale_shift) { set_error("plx_apply_affine: NULL scale/shift"); return PLX_ERR_INVALID; }
    if (d_src == d_out) { set_error("plx_apply_affine: d_out must not alias d_src (rows are written in a different order)"); return PLX_ERR_INVALID; }
    return apply_common(L, d_src, vd, d_out, d_scale_shift, stream, "plx_apply_affine");
}

int plx_apply(plx_lattice *L, const float *d_src, int vd, float *d_out, void *stream)
{
    return apply_common(L, d_src, vd, d_out, nullptr, stream, "plx_apply");
}

static int affine_dot_tiles(const plx_lattice *L, int vd)
{
    const int64_t n_own = L->own_end - L->own_begin;
    return ceil_div(n_own * (values_stride(vd) / 4), kBlock);
}

int64_t plx_affine_dot_work_floats(const plx_lattice *L, int vd)
{
    if (!L || !L->built || vd < 2 || vd > 256) return -1;
    return (int64_t)affine_dot_tiles(L, vd) * values_stride(vd);
}

int plx_apply_affine_dot(plx_lattice *L, const float *d_src, int vd, float *d_out, const float *d_scale_shift,
                         float *d_dot, float *d_work, void *stream)
{
    EntryScope sc(L, stream);
    if (!d_scale_shift || !d_work) { set_error("plx_apply_affine_dot: NULL argument"); return PLX_ERR_INVALID; }
    if (d_src == d_out) { set_error("plx_apply_affine_dot: d_out must not alias d_src"); return PLX_ERR_INVALID; }
    if (vd < 2 || vd > 256) { set_error("plx_apply_affine_dot: vd = %d outside 2..256 (use plx_apply_affine + plx_coldot)", vd); return PLX_ERR_INVALID; }
    PLX_TRY(check_apply(L, d_src, d_out, vd, "plx_apply_affine_dot"));
    DeviceGuard g(L->device);
    const int vdp = values_stride(vd);
    PLX_TRY(ensure(L->val_a, (size_t)L->m * vdp * 4));
    PLX_TRY(ensure(L->val_b, (size_t)L->m * vdp * 4));
    hipStream_t s = (hipStream_t)stream;
    L->tev_n = 0;
    tmark(L, s);
    PLX_TRY(splat_impl(L, d_src, vd, L->val_a.as<float>(), s));
    int in_b = 0;
    PLX_TRY(blur_impl(L, L->val_a.as<float>(), L->val_b.as<float>(), vd, &in_b, s));
    PLX_TRY(slice_impl(L, in_b ? L->val_b.as<float>() : L->val_a.as<float>(), vd, d_out, s, d_scale_shift, d_src, d_work));
    if (!d_dot) return PLX_OK;          // the per-tile partial sums stay in d_work (plx_cg_step_update_fused adds them up itself)
    return coldot_final(d_work, affine_dot_tiles(L, vd), vdp, vdp, d_dot, s);
}

int plx_affine_dot_tiles(const plx_lattice *L, int vd)
{
    if (!L || !L->built || vd < 2 || vd > 256) return -1;
    return affine_dot_tiles(L, vd);
}

static int apply_common(plx_lattice *L, const float *d_src, int vd, float *d_out, const float *d_affine, void *stream,
                        const char *who)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_apply(L, d_src, d_out, vd, who));
    DeviceGuard g(L->device);
    PLX_TRY(ensure(L->val_a, (size_t)L->m * values_stride(vd) * 4));
    PLX_TRY(ensure(L->val_b, (size_t)L->m * values_stride(vd) * 4));
    hipStream_t s = (hipStream_t)stream;
    L->tev_n = 0;
    tmark(L, s);
    PLX_TRY(splat_impl(L, d_src, vd, L->val_a.as<float>(), s));
    int in_b = 0;
    PLX_TRY(blur_impl(L, L->val_a.as<float>(), L->val_b.as<float>(), vd, &in_b, s));
    return slice_impl(L, in_b ? L->val_b.as<float>() : L->val_a.as<float>(), vd, d_out, s, d_affine, d_src);
}

// ---- the rectangular product: splat / slice by row range (kernels: plx_rows_kernels.h; tables: plx_rows.hip) ----------

// The two checks the rows calls and the fp64 calls share.  A range of caller rows: non-empty, inside [0, n).
static int check_range(const plx_lattice *L, int64_t begin, int64_t count, const char *who)
{
    if (count < 1 || begin < 0 || begin > L->n || count > L->n - begin) {
        set_error("%s: rows [%lld, %lld + %lld) are not a non-empty range inside [0, %lld)", who, (long long)begin,
                  (long long)begin, (long long)count, (long long)L->n);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

// The 2^31 element limits of the gather kernels: m vertex rows and `rows` caller rows (named `rows_name` in the message) of
// `stride` elements each.
static int check_size(const plx_lattice *L, int stride, int64_t rows, const char *rows_name, const char *who)
{
    if ((int64_t)L->m * stride >= (1ll << 31) || rows * stride >= (1ll << 31)) {
        set_error("%s: m*vd or %s*vd exceeds 2^31 elements; split the columns", who, rows_name);
        return PLX_ERR_TOO_LARGE;
    }
    return PLX_OK;
}

// Everything a rows call checks before any GPU work.  `a` / `b`: the call's two buffers.
static int check_rows(const plx_lattice *L, const void *a, const void *b, int vd, int64_t begin, int64_t count,
                      const char *who)
{
    PLX_TRY(check_call(L, a, b, vd, who));
    PLX_TRY(check_range(L, begin, count, who));
    PLX_TRY(check_plain_build(L, "row ranges are", who));
    return check_size(L, values_stride(vd), count, "rows", who);
}

static int check_values_aligned(const void *d_values, int vd, const char *who)
{
    if (vd > 1 && ((uintptr_t)d_values & 15) != 0) {
        set_error("%s: d_values must be 16-byte aligned (vertex rows are whole 16-byte vectors)", who);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

int plx_splat_rows(plx_lattice *L, const float *d_src, int64_t row_begin, int64_t row_count, int vd, float *d_values,
                   void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_rows(L, d_src, d_values, vd, row_begin, row_count, "plx_splat_rows"));
    PLX_TRY(check_values_aligned(d_values, vd, "plx_splat_rows"));
    DeviceGuard g(L->device);
    return splat_rows_impl<float>(L, d_src, row_begin, row_count, vd, d_values, (hipStream_t)stream);
}

int plx_slice_rows(plx_lattice *L, const float *d_values, int vd, int64_t row_begin, int64_t row_count, float *d_out,
                   void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_rows(L, d_values, d_out, vd, row_begin, row_count, "plx_slice_rows"));
    PLX_TRY(check_values_aligned(d_values, vd, "plx_slice_rows"));
    DeviceGuard g(L->device);
    return slice_rows_impl<float>(L, d_values, vd, row_begin, row_count, d_out, (hipStream_t)stream);
}

int plx_apply_rows(plx_lattice *L, const float *d_src, int64_t src_begin, int64_t src_count, int vd, float *d_out,
                   int64_t out_begin, int64_t out_count, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_rows(L, d_src, d_out, vd, src_begin, src_count, "plx_apply_rows (source rows)"));
    PLX_TRY(check_rows(L, d_src, d_out, vd, out_begin, out_count, "plx_apply_rows (output rows)"));
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    PLX_TRY(ensure(L->val_a, (size_t)L->m * values_stride(vd) * 4));
    PLX_TRY(ensure(L->val_b, (size_t)L->m * values_stride(vd) * 4));
    PLX_TRY(splat_rows_impl<float>(L, d_src, src_begin, src_count, vd, L->val_a.as<float>(), s));
    int in_b = 0;
    PLX_TRY(blur_impl(L, L->val_a.as<float>(), L->val_b.as<float>(), vd, &in_b, s));
    return slice_rows_impl<float>(L, in_b ? L->val_b.as<float>() : L->val_a.as<float>(), vd, out_begin, out_count, d_out, s);
}

int plx_last_rows_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) return PLX_ERR_INVALID;
    snprintf(buf, (size_t)cap, "splat=%s;slice=%s", L->kn_rows_splat, L->kn_rows_slice);
    return PLX_OK;
}

// ---- the float64 product (kernels: plx_f64.hip) ------------------------------------------------------------------------

int plx_values_stride_f64(int vd) { return vd >= 1 ? values_stride_f64(vd) : -1; }

static int check_doubles_aligned(const void *a, const void *b, const char *who)
{
    if ((((uintptr_t)a | (uintptr_t)b) & 7) != 0) { set_error("%s: buffers of doubles must be 8-byte aligned", who); return PLX_ERR_INVALID; }
    return PLX_OK;
}

// Everything an fp64 call checks before any GPU work.  `a` / `b`: the call's two buffers of doubles.
static int check_f64(const plx_lattice *L, const void *a, const void *b, int vd, const char *who)
{
    PLX_TRY(check_call(L, a, b, vd, who));
    PLX_TRY(check_doubles_aligned(a, b, who));
    PLX_TRY(check_plain_build(L, "the float64 product is", who));
    return check_size(L, values_stride_f64(vd), L->n, "n", who);
}

int plx_splat_f64(plx_lattice *L, const double *d_src, int vd, double *d_values, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_f64(L, d_src, d_values, vd, "plx_splat_f64"));
    PLX_TRY(check_values_aligned(d_values, vd, "plx_splat_f64"));
    DeviceGuard g(L->device);
    return splat_f64_impl(L, d_src, vd, d_values, (hipStream_t)stream);
}

int plx_blur_f64(plx_lattice *L, double *d_values, double *d_scratch, int vd, int *result_in_scratch, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_f64(L, d_values, d_scratch, vd, "plx_blur_f64"));
    if (!result_in_scratch) { set_error("plx_blur_f64: result_in_scratch is NULL"); return PLX_ERR_INVALID; }
    if (d_values == d_scratch) { set_error("plx_blur_f64: d_values and d_scratch must be different buffers"); return PLX_ERR_INVALID; }
    PLX_TRY(check_values_aligned(d_values, vd, "plx_blur_f64"));
    PLX_TRY(check_values_aligned(d_scratch, vd, "plx_blur_f64"));
    DeviceGuard g(L->device);
    return blur_f64_impl(L, d_values, d_scratch, vd, result_in_scratch, (hipStream_t)stream);
}

int plx_slice_f64(plx_lattice *L, const double *d_values, int vd, double *d_out, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_f64(L, d_values, d_out, vd, "plx_slice_f64"));
    PLX_TRY(check_values_aligned(d_values, vd, "plx_slice_f64"));
    DeviceGuard g(L->device);
    return slice_f64_impl(L, d_values, vd, d_out, (hipStream_t)stream);
}

int plx_apply_f64(plx_lattice *L, const double *d_src, int vd, double *d_out, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_f64(L, d_src, d_out, vd, "plx_apply_f64"));
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    PLX_TRY(ensure(L->val64_a, (size_t)L->m * values_stride_f64(vd) * 8));
    PLX_TRY(ensure(L->val64_b, (size_t)L->m * values_stride_f64(vd) * 8));
    PLX_TRY(splat_f64_impl(L, d_src, vd, L->val64_a.as<double>(), s));
    int in_b = 0;
    PLX_TRY(blur_f64_impl(L, L->val64_a.as<double>(), L->val64_b.as<double>(), vd, &in_b, s));
    return slice_f64_impl(L, in_b ? L->val64_b.as<double>() : L->val64_a.as<double>(), vd, d_out, s);
}

// ---- the float64 affine product of a CG iteration (slice + tail + dot: plx_cg_f64.hip) --------------------------------------
int64_t plx_affine_dot_work_doubles(const plx_lattice *L, int vd)
{
    if (!L || !L->built || vd < 1) return -1;
    const int rows = affine_f64_dot_rows(L, vd);
    return rows > 0 ? (int64_t)rows * values_stride_f64(vd) : -1;
}

int plx_apply_affine_f64(plx_lattice *L, const double *d_src, int vd, double *d_out, const double *d_scale_shift, double *d_dot,
                         double *d_work, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_f64(L, d_src, d_out, vd, "plx_apply_affine_f64"));
    if (!d_scale_shift) { set_error("plx_apply_affine_f64: NULL scale/shift"); return PLX_ERR_INVALID; }
    if (d_dot && !d_work) { set_error("plx_apply_affine_f64: d_dot needs d_work (plx_affine_dot_work_doubles)"); return PLX_ERR_INVALID; }
    PLX_TRY(check_doubles_aligned(d_scale_shift, d_dot, "plx_apply_affine_f64"));
    PLX_TRY(check_doubles_aligned(d_work, nullptr, "plx_apply_affine_f64"));
    if (d_src == d_out) { set_error("plx_apply_affine_f64: d_out must not alias d_src"); return PLX_ERR_INVALID; }
    const int dot_rows = d_dot ? affine_f64_dot_rows(L, vd) : 0;
    if (d_dot && dot_rows < 1) {
        set_error("plx_apply_affine_f64: the fused dot serves vd <= 128, got %d (pass d_dot = NULL and use plx_coldot_f64)", vd);
        return PLX_ERR_INVALID;
    }
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    PLX_TRY(ensure(L->val64_a, (size_t)L->m * values_stride_f64(vd) * 8));      // the workspace of plx_apply_f64
    PLX_TRY(ensure(L->val64_b, (size_t)L->m * values_stride_f64(vd) * 8));
    PLX_TRY(splat_f64_impl(L, d_src, vd, L->val64_a.as<double>(), s));
    int in_b = 0;
    PLX_TRY(blur_f64_impl(L, L->val64_a.as<double>(), L->val64_b.as<double>(), vd, &in_b, s));
    PLX_TRY(slice_affine_f64_impl(L, in_b ? L->val64_b.as<double>() : L->val64_a.as<double>(), vd, d_src, d_scale_shift, d_out,
                                  d_dot ? d_work : nullptr, s));
    if (!d_dot) return PLX_OK;
    return coldot_final(d_work, dot_rows, values_stride_f64(vd), vd, d_dot, s);
}

int plx_last_f64_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) return PLX_ERR_INVALID;
    snprintf(buf, (size_t)cap, "splat=%s;blur_axis=%s;slice=%s", L->kn_f64_splat, L->kn_f64_blur, L->kn_f64_slice);
    return PLX_OK;
}

// ---- the transposed and symmetrised products, fp32 and float64 (kernels: plx_sym_kernels.h, instantiated by plx_sym.hip
// and plx_sym_f64.hip, around blur_axis_kernel of plx_blur.hip and the blur kernels of plx_f64.hip) -------------------------

// Everything a transposed or symmetrised fp32 call checks before any GPU work.  `a` / `b`: the call's two buffers.
static int check_sym32(const plx_lattice *L, const void *a, const void *b, int vd, const char *who)
{
    PLX_TRY(check_call(L, a, b, vd, who));
    PLX_TRY(check_plain_build(L, "the transposed and symmetrised products are", who));
    return check_size(L, values_stride(vd), L->n, "n", who);
}

extern "C++" {      // one body per call for both types; the entry points below forward to them

// The stage implementations name their kernels in the fields of the plain calls (kn_f64_*; kn_splat / kn_slice): a
// transposed or symmetrised call moves what it launched to its own fields (kn_sym_*; kn_sym32_*) and leaves
// plx_last_f64_kernels / plx_last_kernels with what the last plain call reported.  `blur`: the name of the blur where no
// stage assigns one -- the dual kernel's, and in fp32 the transposed blur's too: nothing these calls run assigns kn_blur,
// which is not borrowed (a NULL field).
using KnField = const char *plx_lattice::*;
struct SymKernelNames {
    plx_lattice *L;
    const KnField *plain, *sym;      // splat, blur, slice
    const char *saved[3] = {};
    SymKernelNames(plx_lattice *lat, const KnField *plain_, const KnField *sym_, const char *blur) : L(lat), plain(plain_), sym(sym_)
    {
        for (int i = 0; i < 3; ++i) {
            L->*sym[i] = "";
            if (!plain[i]) continue;
            saved[i] = L->*plain[i];
            L->*plain[i] = "";
        }
        L->*sym[1] = blur;
    }
    ~SymKernelNames()
    {
        for (int i = 0; i < 3; ++i) {
            if (!plain[i]) continue;
            if (*(L->*plain[i])) L->*sym[i] = L->*plain[i];
            L->*plain[i] = saved[i];
        }
    }
};

template <typename T> static bool overlap(const T *a, int64_t na, const T *b, int64_t nb)
{
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

// What the two types differ in here: the argument check, the workspace, the stage implementations, the name fields and
// the names, and the aliasing rule of the transposed blur.
template <typename T> struct SymHost;
template <> struct SymHost<double> {
    static constexpr KnField kPlain[3] = {&plx_lattice::kn_f64_splat, &plx_lattice::kn_f64_blur, &plx_lattice::kn_f64_slice};
    static constexpr KnField kSym[3] = {&plx_lattice::kn_sym_splat, &plx_lattice::kn_sym_blur, &plx_lattice::kn_sym_slice};
    static constexpr const char *kBlurT = "", *kDual = "f64_blur_dual_kernel", *kWorkSize = "plx_blur_sym_work_doubles";
    static constexpr const char *kScratchRule = "must be different buffers";      // plx_blur_t_f64 refuses d_values == d_scratch only
    static constexpr bool kScratchMayOverlap = true;
    static constexpr DevBuf plx_lattice::*kValA = &plx_lattice::val64_a, plx_lattice::*kValB = &plx_lattice::val64_b,
                                        plx_lattice::*kValS = &plx_lattice::val64_s;      // a, b: the workspace of plx_apply_f64
    static constexpr auto check = check_f64; static constexpr auto stride = values_stride_f64;
    static constexpr auto splat = splat_f64_impl; static constexpr auto slice = slice_f64_impl;
    static constexpr auto blur_t = blur_t_f64_impl; static constexpr auto blur_sym = blur_sym_f64_impl;
};
template <> struct SymHost<float> {
    static constexpr KnField kPlain[3] = {&plx_lattice::kn_splat, nullptr, &plx_lattice::kn_slice};
    static constexpr KnField kSym[3] = {&plx_lattice::kn_sym32_splat, &plx_lattice::kn_sym32_blur, &plx_lattice::kn_sym32_slice};
    static constexpr const char *kBlurT = "blur_axis_kernel", *kDual = "blur_dual_kernel", *kWorkSize = "plx_blur_sym_work_floats";
    static constexpr const char *kScratchRule = "must not overlap";      // plx_blur_t refuses any overlap of the two planes
    static constexpr bool kScratchMayOverlap = false;
    static constexpr DevBuf plx_lattice::*kValA = &plx_lattice::val_a, plx_lattice::*kValB = &plx_lattice::val_b,
                                        plx_lattice::*kValS = &plx_lattice::val_s;      // a, b: the workspace of plx_apply
    static constexpr auto check = check_sym32; static constexpr auto stride = values_stride;
    static constexpr auto blur_t = blur_t_impl; static constexpr auto blur_sym = blur_sym_impl;
    static constexpr auto splat = splat_impl;      // (slice_impl has trailing arguments with defaults: a function of its own)
    static int slice(plx_lattice *L, const float *d_values, int vd, float *d_out, hipStream_t s) { return slice_impl(L, d_values, vd, d_out, s); }
};

template <typename T>
static int blur_t_entry(const char *who, plx_lattice *L, T *d_values, T *d_scratch, int vd, int *result_in_scratch, void *stream)
{
    using S = SymHost<T>;
    EntryScope sc(L, stream);
    PLX_TRY(S::check(L, d_values, d_scratch, vd, who));
    if (!result_in_scratch) { set_error("%s: result_in_scratch is NULL", who); return PLX_ERR_INVALID; }
    const int64_t plane = (int64_t)L->m * S::stride(vd);
    if (S::kScratchMayOverlap ? d_values == d_scratch : overlap(d_values, plane, d_scratch, plane)) {
        set_error("%s: d_values and d_scratch %s", who, S::kScratchRule);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_values_aligned(d_values, vd, who));
    PLX_TRY(check_values_aligned(d_scratch, vd, who));
    DeviceGuard g(L->device);
    SymKernelNames kn(L, S::kPlain, S::kSym, S::kBlurT);
    return S::blur_t(L, d_values, d_scratch, vd, result_in_scratch, (hipStream_t)stream);
}

template <typename T> static int apply_t_entry(const char *who, plx_lattice *L, const T *d_src, int vd, T *d_out, void *stream)
{
    using S = SymHost<T>;
    EntryScope sc(L, stream);
    PLX_TRY(S::check(L, d_src, d_out, vd, who));
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)L->m * S::stride(vd) * sizeof(T);
    PLX_TRY(ensure(L->*S::kValA, bytes));
    PLX_TRY(ensure(L->*S::kValB, bytes));
    T *va = (L->*S::kValA).template as<T>(), *vb = (L->*S::kValB).template as<T>();
    SymKernelNames kn(L, S::kPlain, S::kSym, S::kBlurT);
    PLX_TRY(S::splat(L, d_src, vd, va, s));
    int in_b = 0;
    PLX_TRY(S::blur_t(L, va, vb, vd, &in_b, s));
    return S::slice(L, in_b ? vb : va, vd, d_out, s);
}

template <typename T>
static int blur_sym_entry(const char *who, plx_lattice *L, T *d_values, T *d_work, int vd, T **d_result, void *stream)
{
    using S = SymHost<T>;
    EntryScope sc(L, stream);
    PLX_TRY(S::check(L, d_values, d_work, vd, who));
    if (!d_result) { set_error("%s: d_result is NULL", who); return PLX_ERR_INVALID; }
    const int64_t plane = (int64_t)L->m * S::stride(vd);
    if (overlap(d_values, plane, d_work, blur_sym_planes(L) * plane)) {
        set_error("%s: d_values and d_work (%s) must not overlap", who, S::kWorkSize);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_values_aligned(d_values, vd, who));
    PLX_TRY(check_values_aligned(d_work, vd, who));
    DeviceGuard g(L->device);
    SymKernelNames kn(L, S::kPlain, S::kSym, S::kDual);
    T *planes[3] = {d_work, d_work + plane, d_work + 2 * plane};      // (the last ones unused where d + 1 < 3)
    return S::blur_sym(L, d_values, planes, vd, d_result, (hipStream_t)stream);
}

// splat + symmetrised blur on the lattice's workspace of the type: plane a holds the splat, plane b and the two planes of
// val_s / val64_s are the work space; *d_blurred: the plane the slice reads
template <typename T> static int splat_blur_sym(plx_lattice *L, const T *d_src, int vd, T **d_blurred, hipStream_t s)
{
    using S = SymHost<T>;
    const size_t plane = (size_t)L->m * S::stride(vd);
    PLX_TRY(ensure(L->*S::kValA, plane * sizeof(T)));
    PLX_TRY(ensure(L->*S::kValB, plane * sizeof(T)));
    PLX_TRY(ensure(L->*S::kValS, 2 * plane * sizeof(T)));
    T *va = (L->*S::kValA).template as<T>(), *vs = (L->*S::kValS).template as<T>();
    PLX_TRY(S::splat(L, d_src, vd, va, s));
    // the three work planes need not be contiguous here: the symmetrised blur takes them one by one
    T *planes[3] = {(L->*S::kValB).template as<T>(), vs, vs + plane};
    return S::blur_sym(L, va, planes, vd, d_blurred, s);
}

template <typename T> static int apply_sym_entry(const char *who, plx_lattice *L, const T *d_src, int vd, T *d_out, void *stream)
{
    using S = SymHost<T>;
    EntryScope sc(L, stream);
    PLX_TRY(S::check(L, d_src, d_out, vd, who));
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    SymKernelNames kn(L, S::kPlain, S::kSym, S::kDual);
    T *blurred = nullptr;
    PLX_TRY(splat_blur_sym<T>(L, d_src, vd, &blurred, s));
    return S::slice(L, blurred, vd, d_out, s);
}

}  // extern "C++"

int plx_blur_t_f64(plx_lattice *L, double *d_values, double *d_scratch, int vd, int *result_in_scratch, void *stream)
{
    return blur_t_entry<double>("plx_blur_t_f64", L, d_values, d_scratch, vd, result_in_scratch, stream);
}

int plx_apply_t_f64(plx_lattice *L, const double *d_src, int vd, double *d_out, void *stream)
{
    return apply_t_entry<double>("plx_apply_t_f64", L, d_src, vd, d_out, stream);
}

int64_t plx_blur_sym_work_doubles(const plx_lattice *L, int vd)
{
    if (!L || !L->built || vd < 1) return -1;
    return (int64_t)blur_sym_f64_planes(L) * L->m * values_stride_f64(vd);
}

int plx_blur_sym_f64(plx_lattice *L, double *d_values, double *d_work, int vd, double **d_result, void *stream)
{
    return blur_sym_entry<double>("plx_blur_sym_f64", L, d_values, d_work, vd, d_result, stream);
}

int plx_apply_sym_f64(plx_lattice *L, const double *d_src, int vd, double *d_out, void *stream)
{
    return apply_sym_entry<double>("plx_apply_sym_f64", L, d_src, vd, d_out, stream);
}

int plx_apply_affine_sym_f64(plx_lattice *L, const double *d_src, int vd, double *d_out, const double *d_scale_shift, double *d_dot,
                             double *d_work, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_f64(L, d_src, d_out, vd, "plx_apply_affine_sym_f64"));
    if (!d_scale_shift) { set_error("plx_apply_affine_sym_f64: NULL scale/shift"); return PLX_ERR_INVALID; }
    if (d_dot && !d_work) { set_error("plx_apply_affine_sym_f64: d_dot needs d_work (plx_affine_dot_work_doubles)"); return PLX_ERR_INVALID; }
    PLX_TRY(check_doubles_aligned(d_scale_shift, d_dot, "plx_apply_affine_sym_f64"));
    PLX_TRY(check_doubles_aligned(d_work, nullptr, "plx_apply_affine_sym_f64"));
    if (d_src == d_out) { set_error("plx_apply_affine_sym_f64: d_out must not alias d_src"); return PLX_ERR_INVALID; }
    const int dot_rows = d_dot ? affine_f64_dot_rows(L, vd) : 0;
    if (d_dot && dot_rows < 1) {
        set_error("plx_apply_affine_sym_f64: the fused dot serves vd <= 128, got %d (pass d_dot = NULL and use plx_coldot_f64)", vd);
        return PLX_ERR_INVALID;
    }
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    SymKernelNames kn(L, SymHost<double>::kPlain, SymHost<double>::kSym, SymHost<double>::kDual);
    double *blurred = nullptr;
    PLX_TRY(splat_blur_sym<double>(L, d_src, vd, &blurred, s));
    PLX_TRY(slice_affine_f64_impl(L, blurred, vd, d_src, d_scale_shift, d_out, d_dot ? d_work : nullptr, s));
    if (!d_dot) return PLX_OK;
    return coldot_final(d_work, dot_rows, values_stride_f64(vd), vd, d_dot, s);
}

int plx_last_sym_f64_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) return PLX_ERR_INVALID;
    snprintf(buf, (size_t)cap, "splat=%s;blur=%s;slice=%s", L->kn_sym_splat, L->kn_sym_blur, L->kn_sym_slice);
    return PLX_OK;
}

// ... and the fp32 ones
int plx_blur_t(plx_lattice *L, float *d_values, float *d_scratch, int vd, int *result_in_scratch, void *stream)
{
    return blur_t_entry<float>("plx_blur_t", L, d_values, d_scratch, vd, result_in_scratch, stream);
}

int plx_apply_t(plx_lattice *L, const float *d_src, int vd, float *d_out, void *stream)
{
    return apply_t_entry<float>("plx_apply_t", L, d_src, vd, d_out, stream);
}

int64_t plx_blur_sym_work_floats(const plx_lattice *L, int vd)
{
    if (!L || !L->built || vd < 1) return -1;
    return (int64_t)blur_sym_planes(L) * L->m * values_stride(vd);
}

int plx_blur_sym(plx_lattice *L, float *d_values, float *d_work, int vd, float **d_result, void *stream)
{
    return blur_sym_entry<float>("plx_blur_sym", L, d_values, d_work, vd, d_result, stream);
}

int plx_apply_sym(plx_lattice *L, const float *d_src, int vd, float *d_out, void *stream)
{
    return apply_sym_entry<float>("plx_apply_sym", L, d_src, vd, d_out, stream);
}

int plx_apply_affine_sym(plx_lattice *L, const float *d_src, int vd, float *d_out, const float *d_scale_shift, float *d_dot,
                         float *d_work, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_sym32(L, d_src, d_out, vd, "plx_apply_affine_sym"));
    if (!d_scale_shift) { set_error("plx_apply_affine_sym: NULL scale/shift"); return PLX_ERR_INVALID; }
    if (d_dot && !d_work) { set_error("plx_apply_affine_sym: d_dot needs d_work (plx_affine_dot_work_floats)"); return PLX_ERR_INVALID; }
    if (d_src == d_out) { set_error("plx_apply_affine_sym: d_out must not alias d_src (rows are written in a different order)"); return PLX_ERR_INVALID; }
    if (d_work && (vd < 2 || vd > 256)) {
        set_error("plx_apply_affine_sym: the fused dot serves vd in 2..256, got %d (pass d_work = NULL and use plx_coldot)", vd);
        return PLX_ERR_INVALID;
    }
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    SymKernelNames kn(L, SymHost<float>::kPlain, SymHost<float>::kSym, SymHost<float>::kDual);
    float *blurred = nullptr;
    PLX_TRY(splat_blur_sym<float>(L, d_src, vd, &blurred, s));
    PLX_TRY(slice_impl(L, blurred, vd, d_out, s, d_scale_shift, d_src, d_work));
    if (!d_dot) return PLX_OK;          // d_work set: the per-tile partial sums stay there (plx_cg_step_update_fused adds them up)
    return coldot_final(d_work, affine_dot_tiles(L, vd), values_stride(vd), values_stride(vd), d_dot, s);
}

int plx_last_sym_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) return PLX_ERR_INVALID;
    snprintf(buf, (size_t)cap, "splat=%s;blur=%s;slice=%s", L->kn_sym32_splat, L->kn_sym32_blur, L->kn_sym32_slice);
    return PLX_OK;
}

// ---- the true diagonal K_ii (kernel: plx_diag_kernels.h, instantiated by plx_diag.hip and plx_diag_f64.hip) ------------

// Everything a diagonal call checks before its one launch.  `align`: bytes of an output element.
static int check_diag(const plx_lattice *L, const void *d_out, int64_t begin, int64_t count, int lattice_rows, size_t align,
                      const char *who)
{
    if (!L || !d_out) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (!L->built) { set_error("%s: lattice not built", who); return PLX_ERR_STATE; }
    if (((uintptr_t)d_out & (align - 1)) != 0) {
        set_error("%s: d_out must be %d-byte aligned", who, (int)align);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_range(L, begin, count, who));
    if (lattice_rows && (begin != 0 || count != L->n)) {
        set_error("%s: lattice_rows serves the whole range [0, %lld) only", who, (long long)L->n);
        return PLX_ERR_INVALID;
    }
    return check_plain_build(L, "the diagonal is", who);
}

int plx_diag(plx_lattice *L, int64_t row_begin, int64_t row_count, int lattice_rows, float *d_out, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_diag(L, d_out, row_begin, row_count, lattice_rows, sizeof(float), "plx_diag"));
    DeviceGuard g(L->device);
    return diag_impl<float>(L, row_begin, row_count, lattice_rows != 0, d_out, (hipStream_t)stream);
}

int plx_diag_f64(plx_lattice *L, int64_t row_begin, int64_t row_count, int lattice_rows, double *d_out, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_diag(L, d_out, row_begin, row_count, lattice_rows, sizeof(double), "plx_diag_f64"));
    DeviceGuard g(L->device);
    return diag_impl<double>(L, row_begin, row_count, lattice_rows != 0, d_out, (hipStream_t)stream);
}

// ---- queries at foreign points (locate_kernel: plx_build.hip; the slices: plx_query_kernels.h) --------------------------

// What every query call checks about the lattice: built, plain, and not the single-use lattice of plx_filter.
static int check_query_lattice(const plx_lattice *L, const char *who)
{
    if (!L->built) { set_error("%s: lattice not built", who); return PLX_ERR_STATE; }
    PLX_TRY(check_plain_build(L, "queries are", who));
    if (L->single_use) {
        set_error("%s: this lattice was built by plx_filter for one product; queries are served by plx_build lattices", who);
        return PLX_ERR_STATE;
    }
    return PLX_OK;
}

// [a, a + na) and [b, b + nb) share a byte
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

int plx_locate(plx_lattice *L, const float *d_x, int64_t nq, int32_t *d_vid, float *d_w, float *d_mass, void *stream)
{
    const char *who = "plx_locate";
    EntryScope sc(L, stream);
    if (!L || !d_x || !d_vid || !d_w) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (nq < 1) { set_error("%s: nq = %lld must be positive", who, (long long)nq); return PLX_ERR_INVALID; }
    if ((((uintptr_t)d_x | (uintptr_t)d_vid | (uintptr_t)d_w | (uintptr_t)d_mass) & 3) != 0) {
        set_error("%s: buffers must be 4-byte aligned", who);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_query_lattice(L, who));
    const int d1 = L->d + 1;
    if (nq * d1 >= (1ll << 31)) { set_error("%s: nq*(d+1) exceeds 2^31 elements; split the queries", who); return PLX_ERR_TOO_LARGE; }
    const size_t nx = (size_t)nq * L->d * 4, ne = (size_t)nq * d1 * 4, nm = (size_t)nq * 4;
    if (ranges_overlap(d_x, nx, d_vid, ne) || ranges_overlap(d_x, nx, d_w, ne) || ranges_overlap(d_vid, ne, d_w, ne) ||
        (d_mass && (ranges_overlap(d_x, nx, d_mass, nm) || ranges_overlap(d_vid, ne, d_mass, nm) ||
                    ranges_overlap(d_w, ne, d_mass, nm)))) {
        set_error("%s: the outputs must not overlap the queries or each other", who);
        return PLX_ERR_INVALID;
    }
    DeviceGuard g(L->device);
    return locate_impl(L, d_x, nq, d_vid, d_w, d_mass, (hipStream_t)stream);
}

// Everything a slice_at call checks before its one launch.  `esz`: bytes of a value; `stride`: elements of a vertex row.
static int check_slice_at(const plx_lattice *L, const void *d_values, int vd, const void *d_vid, const void *d_w, int64_t nq,
                          const void *d_out, size_t esz, int stride, const char *who)
{
    if (!L || !d_values || !d_vid || !d_w || !d_out) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (nq < 1) { set_error("%s: nq = %lld must be positive", who, (long long)nq); return PLX_ERR_INVALID; }
    if (vd < 1) { set_error("%s: vd = %d must be positive", who, vd); return PLX_ERR_INVALID; }
    if ((((uintptr_t)d_vid | (uintptr_t)d_w) & 3) != 0 || (((uintptr_t)d_values | (uintptr_t)d_out) & (esz - 1)) != 0) {
        set_error("%s: buffers must be aligned to their element size", who);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_values_aligned(d_values, vd, who));
    PLX_TRY(check_query_lattice(L, who));
    PLX_TRY(check_size(L, stride, nq, "nq", who));
    const size_t no = (size_t)nq * vd * esz, ne = (size_t)nq * (L->d + 1) * 4, nv = (size_t)L->m * stride * esz;
    if (ranges_overlap(d_out, no, d_values, nv) || ranges_overlap(d_out, no, d_vid, ne) || ranges_overlap(d_out, no, d_w, ne)) {
        set_error("%s: d_out must not overlap d_values, d_vid or d_w", who);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

int plx_slice_at(plx_lattice *L, const float *d_values, int vd, const int32_t *d_vid, const float *d_w, int64_t nq, float *d_out,
                 void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_slice_at(L, d_values, vd, d_vid, d_w, nq, d_out, sizeof(float), vd >= 1 ? values_stride(vd) : 1, "plx_slice_at"));
    DeviceGuard g(L->device);
    return slice_at_impl<float>(L, d_values, vd, d_vid, d_w, nq, d_out, (hipStream_t)stream);
}

int plx_slice_at_f64(plx_lattice *L, const double *d_values, int vd, const int32_t *d_vid, const float *d_w, int64_t nq,
                     double *d_out, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_slice_at(L, d_values, vd, d_vid, d_w, nq, d_out, sizeof(double), vd >= 1 ? values_stride_f64(vd) : 1,
                           "plx_slice_at_f64"));
    DeviceGuard g(L->device);
    return slice_at_impl<double>(L, d_values, vd, d_vid, d_w, nq, d_out, (hipStream_t)stream);
}

// Everything a slice_at_dots call checks before its one launch: check_slice_at with the upstream gradient in the place of
// the weights and the [d + 1][nq] dots in the place of the output.
static int check_slice_at_dots(const plx_lattice *L, const void *d_values, int vd, const void *d_vid, const void *d_gout,
                               int64_t nq, const void *d_t, size_t esz, int stride, const char *who)
{
    if (!L || !d_values || !d_vid || !d_gout || !d_t) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (nq < 1) { set_error("%s: nq = %lld must be positive", who, (long long)nq); return PLX_ERR_INVALID; }
    if (vd < 1) { set_error("%s: vd = %d must be positive", who, vd); return PLX_ERR_INVALID; }
    if (((uintptr_t)d_vid & 3) != 0 || (((uintptr_t)d_values | (uintptr_t)d_gout | (uintptr_t)d_t) & (esz - 1)) != 0) {
        set_error("%s: buffers must be aligned to their element size", who);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_values_aligned(d_values, vd, who));
    PLX_TRY(check_query_lattice(L, who));
    PLX_TRY(check_size(L, stride, nq, "nq", who));
    const int d1 = L->d + 1;
    if (nq * d1 >= (1ll << 31)) { set_error("%s: nq*(d+1) exceeds 2^31 elements; split the queries", who); return PLX_ERR_TOO_LARGE; }
    const size_t nt = (size_t)nq * d1 * esz, ng = (size_t)nq * vd * esz, ne = (size_t)nq * d1 * 4, nv = (size_t)L->m * stride * esz;
    if (ranges_overlap(d_t, nt, d_values, nv) || ranges_overlap(d_t, nt, d_vid, ne) || ranges_overlap(d_t, nt, d_gout, ng)) {
        set_error("%s: d_t must not overlap d_values, d_vid or d_gout", who);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

int plx_slice_at_dots(plx_lattice *L, const float *d_values, int vd, const int32_t *d_vid, const float *d_gout, int64_t nq,
                      float *d_t, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_slice_at_dots(L, d_values, vd, d_vid, d_gout, nq, d_t, sizeof(float), vd >= 1 ? values_stride(vd) : 1,
                                "plx_slice_at_dots"));
    DeviceGuard g(L->device);
    return slice_at_dots_impl<float>(L, d_values, vd, d_vid, d_gout, nq, d_t, (hipStream_t)stream);
}

int plx_slice_at_dots_f64(plx_lattice *L, const double *d_values, int vd, const int32_t *d_vid, const double *d_gout, int64_t nq,
                          double *d_t, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_slice_at_dots(L, d_values, vd, d_vid, d_gout, nq, d_t, sizeof(double), vd >= 1 ? values_stride_f64(vd) : 1,
                                "plx_slice_at_dots_f64"));
    DeviceGuard g(L->device);
    return slice_at_dots_impl<double>(L, d_values, vd, d_vid, d_gout, nq, d_t, (hipStream_t)stream);
}

// Everything a locate_pullback call checks before its one launch.  `esz`: bytes of an element of d_t and d_gx.
static int check_locate_pullback(const plx_lattice *L, const void *d_x, const void *d_t, int64_t nq, const void *d_gx, size_t esz,
                                 const char *who)
{
    if (!L || !d_x || !d_t || !d_gx) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (nq < 1) { set_error("%s: nq = %lld must be positive", who, (long long)nq); return PLX_ERR_INVALID; }
    if (((uintptr_t)d_x & 3) != 0 || (((uintptr_t)d_t | (uintptr_t)d_gx) & (esz - 1)) != 0) {
        set_error("%s: buffers must be aligned to their element size", who);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_query_lattice(L, who));
    const int d1 = L->d + 1;
    if (nq * d1 >= (1ll << 31)) { set_error("%s: nq*(d+1) exceeds 2^31 elements; split the queries", who); return PLX_ERR_TOO_LARGE; }
    const size_t nx = (size_t)nq * L->d * 4, nt = (size_t)nq * d1 * esz, ng = (size_t)nq * L->d * esz;
    if (ranges_overlap(d_gx, ng, d_x, nx) || ranges_overlap(d_gx, ng, d_t, nt)) {
        set_error("%s: d_gx must not overlap d_x or d_t", who);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

int plx_locate_pullback(plx_lattice *L, const float *d_x, const float *d_t, int64_t nq, float *d_gx, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_locate_pullback(L, d_x, d_t, nq, d_gx, sizeof(float), "plx_locate_pullback"));
    DeviceGuard g(L->device);
    return locate_pullback_impl<float>(L, d_x, d_t, nq, d_gx, (hipStream_t)stream);
}

int plx_locate_pullback_f64(plx_lattice *L, const float *d_x, const double *d_t, int64_t nq, double *d_gx, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_locate_pullback(L, d_x, d_t, nq, d_gx, sizeof(double), "plx_locate_pullback_f64"));
    DeviceGuard g(L->device);
    return locate_pullback_impl<double>(L, d_x, d_t, nq, d_gx, (hipStream_t)stream);
}

int plx_last_query_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) return PLX_ERR_INVALID;
    snprintf(buf, (size_t)cap, "locate=%s;slice_at=%s;dots=%s;pullback=%s", L->kn_locate, L->kn_slice_at, L->kn_dots,
             L->kn_pullback);
    return PLX_OK;
}

// ---- the splat at query points (plx_query_adjoint.hip) -------------------------------------------------------------------

// nq (d + 1) corner pairs within the sort's limit
static int check_plan_pairs(const plx_lattice *L, int64_t nq, const char *who)
{
    if (nq * (L->d + 1) >= (1ll << 31) - 4096) {
        set_error("%s: nq*(d+1) exceeds the 2^31 - 4096 pairs one sort takes; split the queries", who);
        return PLX_ERR_TOO_LARGE;
    }
    return PLX_OK;
}

int64_t plx_query_plan_bytes(const plx_lattice *L, int64_t nq)
{
    if (!L || !L->built || nq < 1 || nq * (L->d + 1) >= (1ll << 31) - 4096) return -1;
    return query_plan_bytes(L->m, L->d, nq);
}

int plx_query_plan(plx_lattice *L, const int32_t *d_vid, const float *d_w, int64_t nq, void *d_plan, void *stream)
{
    const char *who = "plx_query_plan";
    EntryScope sc(L, stream);
    if (!L || !d_vid || !d_w || !d_plan) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (nq < 1) { set_error("%s: nq = %lld must be positive", who, (long long)nq); return PLX_ERR_INVALID; }
    if ((((uintptr_t)d_vid | (uintptr_t)d_w) & 3) != 0 || ((uintptr_t)d_plan & 15) != 0) {
        set_error("%s: d_vid and d_w must be 4-byte aligned, d_plan 16-byte aligned", who);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_query_lattice(L, who));
    PLX_TRY(check_plan_pairs(L, nq, who));
    const size_t ne = (size_t)nq * (L->d + 1) * 4, np = (size_t)query_plan_bytes(L->m, L->d, nq);
    if (ranges_overlap(d_plan, np, d_vid, ne) || ranges_overlap(d_plan, np, d_w, ne)) {
        set_error("%s: d_plan must not overlap d_vid or d_w", who);
        return PLX_ERR_INVALID;
    }
    DeviceGuard g(L->device);
    return query_plan_impl(L, d_vid, d_w, nq, d_plan, (hipStream_t)stream);
}

// Everything a splat_at call checks before its one launch.  `esz`: bytes of a value; `stride`: elements of a vertex row.
static int check_splat_at(const plx_lattice *L, const void *d_plan, const void *d_g, int vd, int64_t nq, const void *d_values,
                          size_t esz, int stride, const char *who)
{
    if (!L || !d_plan || !d_g || !d_values) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (nq < 1) { set_error("%s: nq = %lld must be positive", who, (long long)nq); return PLX_ERR_INVALID; }
    if (vd < 1) { set_error("%s: vd = %d must be positive", who, vd); return PLX_ERR_INVALID; }
    if (((uintptr_t)d_plan & 15) != 0 || (((uintptr_t)d_g | (uintptr_t)d_values) & (esz - 1)) != 0) {
        set_error("%s: d_plan must be 16-byte aligned, d_g and d_values aligned to their element size", who);
        return PLX_ERR_INVALID;
    }
    PLX_TRY(check_values_aligned(d_values, vd, who));
    PLX_TRY(check_query_lattice(L, who));
    PLX_TRY(check_size(L, stride, nq, "nq", who));
    PLX_TRY(check_plan_pairs(L, nq, who));
    const size_t ng = (size_t)nq * vd * esz, nv = (size_t)L->m * stride * esz, np = (size_t)query_plan_bytes(L->m, L->d, nq);
    if (ranges_overlap(d_values, nv, d_g, ng) || ranges_overlap(d_values, nv, d_plan, np)) {
        set_error("%s: d_values must not overlap d_g or d_plan", who);
        return PLX_ERR_INVALID;
    }
    return PLX_OK;
}

int plx_splat_at(plx_lattice *L, const void *d_plan, const float *d_g, int vd, int64_t nq, float *d_values, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_splat_at(L, d_plan, d_g, vd, nq, d_values, sizeof(float), vd >= 1 ? values_stride(vd) : 1, "plx_splat_at"));
    DeviceGuard g(L->device);
    return splat_at_impl<float>(L, d_plan, d_g, vd, nq, d_values, (hipStream_t)stream);
}

int plx_splat_at_f64(plx_lattice *L, const void *d_plan, const double *d_g, int vd, int64_t nq, double *d_values, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_splat_at(L, d_plan, d_g, vd, nq, d_values, sizeof(double), vd >= 1 ? values_stride_f64(vd) : 1,
                           "plx_splat_at_f64"));
    DeviceGuard g(L->device);
    return splat_at_impl<double>(L, d_plan, d_g, vd, nq, d_values, (hipStream_t)stream);
}

int plx_last_splat_at_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) return PLX_ERR_INVALID;
    snprintf(buf, (size_t)cap, "plan=%s;splat_at=%s", L->kn_plan, L->kn_splat_at);
    return PLX_OK;
}

// ---- the float64 rectangular product (kernels: plx_rows_kernels.h; tables: plx_rows.hip; blur: plx_f64.hip) ------------

// check_rows and check_f64 in one: the checks of both, each once.
static int check_rows_f64(const plx_lattice *L, const void *a, const void *b, int vd, int64_t begin, int64_t count,
                          const char *who)
{
    PLX_TRY(check_call(L, a, b, vd, who));
    PLX_TRY(check_doubles_aligned(a, b, who));
    PLX_TRY(check_range(L, begin, count, who));
    PLX_TRY(check_plain_build(L, "float64 row ranges are", who));
    return check_size(L, values_stride_f64(vd), count, "rows", who);
}

int plx_splat_rows_f64(plx_lattice *L, const double *d_src, int64_t row_begin, int64_t row_count, int vd, double *d_values,
                       void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_rows_f64(L, d_src, d_values, vd, row_begin, row_count, "plx_splat_rows_f64"));
    PLX_TRY(check_values_aligned(d_values, vd, "plx_splat_rows_f64"));
    DeviceGuard g(L->device);
    return splat_rows_impl<double>(L, d_src, row_begin, row_count, vd, d_values, (hipStream_t)stream);
}

int plx_slice_rows_f64(plx_lattice *L, const double *d_values, int vd, int64_t row_begin, int64_t row_count, double *d_out,
                       void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_rows_f64(L, d_values, d_out, vd, row_begin, row_count, "plx_slice_rows_f64"));
    PLX_TRY(check_values_aligned(d_values, vd, "plx_slice_rows_f64"));
    DeviceGuard g(L->device);
    return slice_rows_impl<double>(L, d_values, vd, row_begin, row_count, d_out, (hipStream_t)stream);
}

int plx_apply_rows_f64(plx_lattice *L, const double *d_src, int64_t src_begin, int64_t src_count, int vd, double *d_out,
                       int64_t out_begin, int64_t out_count, void *stream)
{
    EntryScope sc(L, stream);
    PLX_TRY(check_rows_f64(L, d_src, d_out, vd, src_begin, src_count, "plx_apply_rows_f64 (source rows)"));
    PLX_TRY(check_rows_f64(L, d_src, d_out, vd, out_begin, out_count, "plx_apply_rows_f64 (output rows)"));
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    PLX_TRY(ensure(L->val64_a, (size_t)L->m * values_stride_f64(vd) * 8));      // the workspace of plx_apply_f64
    PLX_TRY(ensure(L->val64_b, (size_t)L->m * values_stride_f64(vd) * 8));
    PLX_TRY(splat_rows_impl<double>(L, d_src, src_begin, src_count, vd, L->val64_a.as<double>(), s));
    int in_b = 0;
    PLX_TRY(blur_f64_impl(L, L->val64_a.as<double>(), L->val64_b.as<double>(), vd, &in_b, s));
    return slice_rows_impl<double>(L, in_b ? L->val64_b.as<double>() : L->val64_a.as<double>(), vd, out_begin, out_count, d_out, s);
}

int plx_last_rows_f64_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) { set_error("plx_last_rows_f64_kernels: NULL argument or no room"); return PLX_ERR_INVALID; }
    snprintf(buf, (size_t)cap, "splat=%s;slice=%s", L->kn_rows64_splat, L->kn_rows64_slice);
    return PLX_OK;
}

// ---- the float64 position gradient (kernels: plx_backward_f64.hip; blur: plx_f64.hip) ------------------------------------

// Everything a float64 position-gradient call checks before any GPU work.  in[0..n_in): the input buffers; out[0..n_out): the
// output buffers, of which only a trailing d_grad_src may be NULL.  What needs no lattice comes first (check_backward_ptrs,
// shared with the row-range form below); then check_f64 on the 2 nrhs (1 + d) columns of the stack, which are whole 16-byte
// rows (the count is even).
static int check_floats_aligned(const void *a, const char *who)
{
    if (((uintptr_t)a & 3) != 0) { set_error("%s: buffers of floats must be 4-byte aligned", who); return PLX_ERR_INVALID; }
    return PLX_OK;
}

static int check_backward_ptrs(const plx_lattice *L, const void *const *in, int n_in, const void *const *out, int n_out,
                               bool last_out_optional, int nrhs, const char *who, bool f64 = true)
{
    if (!L) { set_error("%s: NULL lattice", who); return PLX_ERR_INVALID; }
    for (int i = 0; i < n_in; ++i)
        if (!in[i]) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    for (int o = 0; o < n_out; ++o)
        if (!out[o] && !(last_out_optional && o == n_out - 1)) { set_error("%s: NULL argument", who); return PLX_ERR_INVALID; }
    if (nrhs < 1) { set_error("%s: nrhs = %d must be positive", who, nrhs); return PLX_ERR_INVALID; }
    for (int i = 0; i < n_in; ++i) PLX_TRY(f64 ? check_doubles_aligned(in[i], nullptr, who) : check_floats_aligned(in[i], who));
    for (int o = 0; o < n_out; ++o) PLX_TRY(f64 ? check_doubles_aligned(out[o], nullptr, who) : check_floats_aligned(out[o], who));
    for (int o = 0; o < n_out; ++o) {
        if (!out[o]) continue;
        bool alias = false;
        for (int i = 0; i < n_in; ++i) alias |= out[o] == in[i];
        for (int q = 0; q < o; ++q) alias |= out[o] == out[q];
        if (alias) { set_error("%s: an output buffer must not alias an input or another output", who); return PLX_ERR_INVALID; }
    }
    return PLX_OK;
}

static int check_backward_f64(const plx_lattice *L, const void *const *in, int n_in, const void *const *out, int n_out,
                              bool last_out_optional, int nrhs, const char *who)
{
    PLX_TRY(check_backward_ptrs(L, in, n_in, out, n_out, last_out_optional, nrhs, who));
    const int64_t cols = 2ll * nrhs * (1 + (L->built ? L->d : 0));
    if (L->built && cols > kBackwardF64MaxCols) {
        set_error("%s: nrhs = %d, d = %d is %lld stacked columns; the on-chip row of the contraction holds up to %d", who, nrhs,
                  L->d, (long long)cols, kBackwardF64MaxCols);
        return PLX_ERR_INVALID;
    }
    return check_f64(L, in[0], in[1], (int)cols, who);
}

int plx_backward_splat_f64(plx_lattice *L, const double *d_g, const double *d_src, const double *d_x, int nrhs,
                           double *d_values, void *stream)
{
    EntryScope sc(L, stream);
    const void *in[] = {d_g, d_src, d_x}, *out[] = {d_values};
    PLX_TRY(check_backward_f64(L, in, 3, out, 1, false, nrhs, "plx_backward_splat_f64"));
    PLX_TRY(check_values_aligned(d_values, 2, "plx_backward_splat_f64"));
    DeviceGuard g(L->device);
    return backward_splat_f64_impl(L, d_g, d_src, d_x, nrhs, d_values, (hipStream_t)stream);
}

int plx_backward_contract_f64(plx_lattice *L, const double *d_values, const double *d_g, const double *d_src,
                              const double *d_x, int nrhs, double *d_grad_x, double *d_grad_src, void *stream)
{
    EntryScope sc(L, stream);
    const void *in[] = {d_values, d_g, d_src, d_x}, *out[] = {d_grad_x, d_grad_src};
    PLX_TRY(check_backward_f64(L, in, 4, out, 2, true, nrhs, "plx_backward_contract_f64"));
    PLX_TRY(check_values_aligned(d_values, 2, "plx_backward_contract_f64"));
    DeviceGuard g(L->device);
    return backward_contract_f64_impl(L, d_values, d_g, d_src, d_x, nrhs, d_grad_x, d_grad_src, (hipStream_t)stream);
}

int plx_apply_backward_f64(plx_lattice *L, const double *d_g, const double *d_src, const double *d_x, int nrhs,
                           double *d_grad_x, double *d_grad_src, void *stream)
{
    EntryScope sc(L, stream);
    const void *in[] = {d_g, d_src, d_x}, *out[] = {d_grad_x, d_grad_src};
    PLX_TRY(check_backward_f64(L, in, 3, out, 2, true, nrhs, "plx_apply_backward_f64"));
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)L->m * 2 * nrhs * (1 + L->d) * 8;
    PLX_TRY(ensure(L->val64_a, bytes));      // the workspace of plx_apply_f64
    PLX_TRY(ensure(L->val64_b, bytes));
    PLX_TRY(backward_splat_f64_impl(L, d_g, d_src, d_x, nrhs, L->val64_a.as<double>(), s));
    int in_b = 0;
    PLX_TRY(blur_f64_impl(L, L->val64_a.as<double>(), L->val64_b.as<double>(), 2 * nrhs * (1 + L->d), &in_b, s));
    return backward_contract_f64_impl(L, in_b ? L->val64_b.as<double>() : L->val64_a.as<double>(), d_g, d_src, d_x, nrhs,
                                      d_grad_x, d_grad_src, s);
}

// ---- the position gradient of the rectangular product, one side per call, in fp32 and in float64 (kernels:
// plx_rows_backward_kernels.h; what the types differ in here: RowsBackwardHost<T>, plx_internal.h) --------------------------
extern "C++" {      // one body per call for both types; the six entry points below forward to them

// Everything a one-sided call checks before any GPU work: the pointer checks of check_backward_f64 and the counts, which
// need no lattice, first; then the built lattice, the column limit on the row stride, the ranges, the build and the sizes.
template <typename T>
static int check_backward_rows(const plx_lattice *L, const void *const *in, int n_in, const void *const *out, int n_out,
                               bool last_out_optional, int nrhs, const int64_t (*ranges)[2], int n_ranges, const char *who)
{
    using S = RowsBackwardHost<T>;
    PLX_TRY(check_backward_ptrs(L, in, n_in, out, n_out, last_out_optional, nrhs, who, std::is_same_v<T, double>));
    for (int r = 0; r < n_ranges; ++r)
        if (ranges[r][1] < 1) { set_error("%s: a row count of %lld must be positive", who, (long long)ranges[r][1]); return PLX_ERR_INVALID; }
    if (!L->built) { set_error("%s: lattice not built", who); return PLX_ERR_STATE; }
    const int64_t cols = (int64_t)nrhs * (1 + L->d), stride = (cols + (S::kPack - 1)) & ~(int64_t)(S::kPack - 1);
    if (stride > S::kMaxCols) {
        set_error("%s: nrhs = %d, d = %d is a row of %lld %s; the on-chip row of the contraction holds up to %d", who, nrhs, L->d,
                  (long long)stride, S::kPlural, S::kMaxCols);
        return PLX_ERR_INVALID;
    }
    for (int r = 0; r < n_ranges; ++r) PLX_TRY(check_range(L, ranges[r][0], ranges[r][1], who));
    PLX_TRY(check_plain_build(L, S::kGradientIs, who));
    for (int r = 0; r < n_ranges; ++r) PLX_TRY(check_size(L, (int)stride, ranges[r][1], "rows", who));
    return PLX_OK;
}

template <typename T>
static int backward_splat_rows_entry(const char *who, plx_lattice *L, const T *d_a, int64_t a_begin, int64_t a_count, const T *d_x,
                                     int nrhs, T *d_values, void *stream)
{
    EntryScope sc(L, stream);
    const void *in[] = {d_a, d_x}, *out[] = {d_values};
    const int64_t ranges[][2] = {{a_begin, a_count}};
    PLX_TRY(check_backward_rows<T>(L, in, 2, out, 1, false, nrhs, ranges, 1, who));
    PLX_TRY(check_values_aligned(d_values, 2, who));
    DeviceGuard g(L->device);
    return backward_splat_rows_impl<T>(L, d_a, a_begin, a_count, d_x, nrhs, d_values, (hipStream_t)stream);
}

template <typename T>
static int backward_contract_rows_entry(const char *who, plx_lattice *L, const T *d_values, const T *d_b, int64_t b_begin,
                                        int64_t b_count, const T *d_x, int nrhs, T *d_grad_x, T *d_filtered, void *stream)
{
    EntryScope sc(L, stream);
    const void *in[] = {d_values, d_b, d_x}, *out[] = {d_grad_x, d_filtered};
    const int64_t ranges[][2] = {{b_begin, b_count}};
    PLX_TRY(check_backward_rows<T>(L, in, 3, out, 2, true, nrhs, ranges, 1, who));
    PLX_TRY(check_values_aligned(d_values, 2, who));
    DeviceGuard g(L->device);
    return backward_contract_rows_impl<T>(L, d_values, d_b, b_begin, b_count, d_x, nrhs, d_grad_x, d_filtered, (hipStream_t)stream);
}

// the two around the blur of the type, on the workspace of plx_apply_rows (float) or of plx_apply_f64 (double)
template <typename T>
static int apply_backward_rows_entry(const char *who, plx_lattice *L, const T *d_a, int64_t a_begin, int64_t a_count, const T *d_b,
                                     int64_t b_begin, int64_t b_count, const T *d_x, int nrhs, T *d_grad_x, T *d_filtered,
                                     void *stream)
{
    EntryScope sc(L, stream);
    const void *in[] = {d_a, d_b, d_x}, *out[] = {d_grad_x, d_filtered};
    const int64_t ranges[][2] = {{a_begin, a_count}, {b_begin, b_count}};
    PLX_TRY(check_backward_rows<T>(L, in, 3, out, 2, true, nrhs, ranges, 2, who));
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    const int H = nrhs * (1 + L->d);
    const size_t bytes = (size_t)L->m * RowsBackwardHost<T>::stride(H) * sizeof(T);
    constexpr bool f64 = std::is_same_v<T, double>;
    DevBuf &work_a = f64 ? L->val64_a : L->val_a, &work_b = f64 ? L->val64_b : L->val_b;
    PLX_TRY(ensure(work_a, bytes));
    PLX_TRY(ensure(work_b, bytes));
    T *va = work_a.template as<T>(), *vb = work_b.template as<T>();
    PLX_TRY(backward_rows_tables<T>(L, a_begin, a_count, b_begin, b_count, s));
    PLX_TRY(backward_splat_rows_impl<T>(L, d_a, a_begin, a_count, d_x, nrhs, va, s));
    int in_b = 0;
    if constexpr (f64) {
        PLX_TRY(blur_f64_impl(L, va, vb, H, &in_b, s));
    } else {
        PLX_TRY(blur_impl(L, va, vb, H, &in_b, s));
    }
    return backward_contract_rows_impl<T>(L, in_b ? vb : va, d_b, b_begin, b_count, d_x, nrhs, d_grad_x, d_filtered, s);
}

}  // extern "C++"

int plx_backward_splat_rows_f64(plx_lattice *L, const double *d_a, int64_t a_begin, int64_t a_count, const double *d_x, int nrhs,
                                double *d_values, void *stream)
{
    return backward_splat_rows_entry<double>("plx_backward_splat_rows_f64", L, d_a, a_begin, a_count, d_x, nrhs, d_values, stream);
}

int plx_backward_contract_rows_f64(plx_lattice *L, const double *d_values, const double *d_b, int64_t b_begin, int64_t b_count,
                                   const double *d_x, int nrhs, double *d_grad_x, double *d_filtered, void *stream)
{
    return backward_contract_rows_entry<double>("plx_backward_contract_rows_f64", L, d_values, d_b, b_begin, b_count, d_x, nrhs,
                                                d_grad_x, d_filtered, stream);
}

int plx_apply_backward_rows_f64(plx_lattice *L, const double *d_a, int64_t a_begin, int64_t a_count, const double *d_b,
                                int64_t b_begin, int64_t b_count, const double *d_x, int nrhs, double *d_grad_x,
                                double *d_filtered, void *stream)
{
    return apply_backward_rows_entry<double>("plx_apply_backward_rows_f64", L, d_a, a_begin, a_count, d_b, b_begin, b_count, d_x,
                                             nrhs, d_grad_x, d_filtered, stream);
}

int plx_backward_splat_rows(plx_lattice *L, const float *d_a, int64_t a_begin, int64_t a_count, const float *d_x, int nrhs,
                            float *d_values, void *stream)
{
    return backward_splat_rows_entry<float>("plx_backward_splat_rows", L, d_a, a_begin, a_count, d_x, nrhs, d_values, stream);
}

int plx_backward_contract_rows(plx_lattice *L, const float *d_values, const float *d_b, int64_t b_begin, int64_t b_count,
                               const float *d_x, int nrhs, float *d_grad_x, float *d_filtered, void *stream)
{
    return backward_contract_rows_entry<float>("plx_backward_contract_rows", L, d_values, d_b, b_begin, b_count, d_x, nrhs, d_grad_x,
                                               d_filtered, stream);
}

int plx_apply_backward_rows(plx_lattice *L, const float *d_a, int64_t a_begin, int64_t a_count, const float *d_b, int64_t b_begin,
                            int64_t b_count, const float *d_x, int nrhs, float *d_grad_x, float *d_filtered, void *stream)
{
    return apply_backward_rows_entry<float>("plx_apply_backward_rows", L, d_a, a_begin, a_count, d_b, b_begin, b_count, d_x, nrhs,
                                            d_grad_x, d_filtered, stream);
}

int plx_apply_backward(plx_lattice *L, const float *d_g, const float *d_src, const float *d_ref, int nrhs,
                       float *d_grad_ref, float *d_grad_src, void *stream)
{
    EntryScope sc(L, stream);
    if (!L) { set_error("plx_apply_backward: NULL lattice"); return PLX_ERR_INVALID; }
    if (!L->built) { set_error("plx_apply_backward: lattice not built"); return PLX_ERR_STATE; }
    if (L->n_shards != 1 || L->partial_cover) {
        set_error("plx_apply_backward: single-shard lattices only (a sharded caller needs the vertex all-reduce between splat and blur)");
        return PLX_ERR_STATE;
    }
    if (!d_g || !d_src || !d_ref || !d_grad_ref) { set_error("plx_apply_backward: NULL argument"); return PLX_ERR_INVALID; }
    const int nch = values_stride(2 * nrhs * (1 + L->d)) / 4;
    if (nrhs < 1 || nch < 32 || nch > 128 || 2 * nrhs + L->d + 2 > 64) {
        set_error("plx_apply_backward: nrhs = %d, d = %d (%d columns) is outside the fused kernels' range (125..512 "
                  "columns, 2*nrhs + d <= 62); use plx_backward_stack + plx_apply + plx_backward_contract", nrhs, L->d,
                  2 * nrhs * (1 + L->d));
        return PLX_ERR_INVALID;
    }
    DeviceGuard g(L->device);
    return backward_impl(L, d_g, d_src, d_ref, nrhs, d_grad_ref, d_grad_src, (hipStream_t)stream);
}

int plx_filter(plx_lattice *scratch, const float *d_src, const float *d_ref, int64_t n, int d, int vd,
               const float *h_taps, int ntaps, float *d_out, void *stream)
{
    plx_lattice *L = scratch;
    if (!L) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) { set_error("plx_filter: hipGetDevice failed"); return PLX_ERR_HIP; }
        PLX_TRY(plx_create(dev, &L));
    }
    int rc = build_entry(L, d_ref, n, d, h_taps, ntaps, 0, 1, stream, true);
    if (rc == PLX_OK) rc = plx_apply(L, d_src, vd, d_out, stream);
    if (!scratch) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        plx_destroy(L);
    }
    return rc;
}

int64_t plx_export_bytes(const plx_lattice *L, int which)
{
    if (!L || !L->built) return -1;
    const int64_t n = L->n, m = L->m, d1 = L->d + 1;
    switch (which) {
    case PLX_ARRAY_KEYS: return m * L->d * 2;
    case PLX_ARRAY_ENTRY_VERTEX: return d1 * n * 4;
    case PLX_ARRAY_ENTRY_WEIGHT: return d1 * n * 4;
    case PLX_ARRAY_NEIGHBORS: return d1 * 2 * L->order * m * 4;
    case PLX_ARRAY_ROW_PTR: return (m + 1) * 4;
    case PLX_ARRAY_CSR_POINT: return L->nnz * 4;
    case PLX_ARRAY_CSR_WEIGHT: return L->nnz * 4;
    case PLX_ARRAY_POINT_PERM: return n * 4;
    default: return -1;
    }
}

int plx_export(plx_lattice *L, int which, void *h_dst, int64_t bytes, void *stream)
{
    EntryScope sc(L, stream);
    if (!L || !h_dst) { set_error("plx_export: NULL argument"); return PLX_ERR_INVALID; }
    if (!L->built) { set_error("plx_export: lattice not built"); return PLX_ERR_STATE; }
    const int64_t want = plx_export_bytes(L, which);
    if (want < 0) { set_error("plx_export: unknown array %d", which); return PLX_ERR_INVALID; }
    if (want != bytes) { set_error("plx_export: array %d is %lld bytes, caller gave %lld", which, (long long)want, (long long)bytes); return PLX_ERR_INVALID; }
    if (bytes == 0) return PLX_OK;
    DeviceGuard g(L->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t m = L->m;
    switch (which) {
    case PLX_ARRAY_KEYS: {
        // device keys are packed int16 pairs padded to DW words per vertex
        const int dw = (L->d + 1) / 2;
        std::vector<uint32_t> tmp((size_t)m * dw);
        PLX_HIP_TRY(hipMemcpyAsync(tmp.data(), L->vkeys.p, tmp.size() * 4, hipMemcpyDeviceToHost, s));
        PLX_HIP_TRY(hipStreamSynchronize(s));
        int16_t *dst = (int16_t *)h_dst;
        for (int64_t i = 0; i < m; ++i)
            for (int c = 0; c < L->d; ++c)
                dst[i * L->d + c] = (int16_t)((tmp[i * dw + (c >> 1)] >> ((c & 1) * 16)) & 0xFFFFu);
        return PLX_OK;
    }
    case PLX_ARRAY_NEIGHBORS: {
        // strip the plane padding (mstride -> m)
        const int planes = (L->d + 1) * 2 * L->order;
        PLX_HIP_TRY(hipMemcpy2DAsync(h_dst, (size_t)m * 4, L->nbr.p, (size_t)L->mstride * 4, (size_t)m * 4,
                                     planes, hipMemcpyDeviceToHost, s));
        break;
    }
    case PLX_ARRAY_ENTRY_VERTEX: PLX_HIP_TRY(hipMemcpyAsync(h_dst, L->evid.p, bytes, hipMemcpyDeviceToHost, s)); break;
    case PLX_ARRAY_ENTRY_WEIGHT: PLX_HIP_TRY(hipMemcpyAsync(h_dst, L->ew.p, bytes, hipMemcpyDeviceToHost, s)); break;
    case PLX_ARRAY_ROW_PTR:
        PLX_TRY(export_row_ptr(L, s));
        PLX_HIP_TRY(hipMemcpyAsync(h_dst, L->row_ptr.p, bytes, hipMemcpyDeviceToHost, s));
        break;
    case PLX_ARRAY_CSR_POINT: {
        PLX_TRY(ensure_csr(L, s));
        PLX_HIP_TRY(hipMemcpyAsync(h_dst, L->csr_pt.p, bytes, hipMemcpyDeviceToHost, s));
        PLX_HIP_TRY(hipStreamSynchronize(s));
        int32_t *dst = (int32_t *)h_dst;   // strip the segment-head flag kept in the sign bit
        for (int64_t i = 0; i < bytes / 4; ++i) dst[i] &= 0x7FFFFFFF;
        return PLX_OK;
    }
    case PLX_ARRAY_CSR_WEIGHT:
        PLX_TRY(ensure_csr(L, s));
        PLX_HIP_TRY(hipMemcpyAsync(h_dst, L->csr_w.p, bytes, hipMemcpyDeviceToHost, s));
        break;
    case PLX_ARRAY_POINT_PERM: PLX_HIP_TRY(hipMemcpyAsync(h_dst, L->perm.p, bytes, hipMemcpyDeviceToHost, s)); break;
    }
    PLX_HIP_TRY(hipStreamSynchronize(s));
    return PLX_OK;
}

int plx_tune(const char *key, int value)
{
    if (!key) return PLX_ERR_INVALID;
    for (const Tunable *t = tunables(); t->name; ++t)
        if (strcmp(t->name, key) == 0) { g_tune_defaults.*(t->member) = value; return PLX_OK; }
    set_error("plx_tune: unknown key %s", key);
    return PLX_ERR_INVALID;
}

int plx_lattice_tune(plx_lattice *L, const char *key, int value)
{
    if (!L || !key) { set_error("plx_lattice_tune: NULL argument"); return PLX_ERR_INVALID; }
    for (const Tunable *t = tunables(); t->name; ++t)
        if (strcmp(t->name, key) == 0) { L->tn.*(t->member) = value; return PLX_OK; }
    set_error("plx_lattice_tune: unknown key %s", key);
    return PLX_ERR_INVALID;
}

int plx_copy_point_perm(plx_lattice *L, void *d_dst, void *stream)
{
    if (!L || !d_dst) { set_error("plx_copy_point_perm: NULL argument"); return PLX_ERR_INVALID; }
    if (!L->built) { set_error("plx_copy_point_perm: lattice not built"); return PLX_ERR_STATE; }
    DeviceGuard g(L->device);
    PLX_HIP_TRY(hipMemcpyAsync(d_dst, L->perm.p, (size_t)L->n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PLX_OK;
}

int plx_set_timing(plx_lattice *L, int on)
{
    if (!L) return PLX_ERR_INVALID;
    L->timing = on != 0;
    return PLX_OK;
}

int plx_apply_times(plx_lattice *L, float *h_ms, int cap, int *count)
{
    if (!L || !h_ms || !count) return PLX_ERR_INVALID;
    *count = 0;
    if (!L->timing || L->tev_n < 2) return PLX_OK;
    DeviceGuard g(L->device);
    PLX_HIP_TRY(hipEventSynchronize(L->tev[L->tev_n - 1]));
    const int k = L->tev_n - 1;
    for (int i = 0; i < k && i < cap; ++i) PLX_HIP_TRY(hipEventElapsedTime(&h_ms[i], L->tev[i], L->tev[i + 1]));
    *count = k < cap ? k : cap;
    return PLX_OK;
}

int plx_last_kernels(const plx_lattice *L, char *buf, int cap)
{
    if (!L || !buf || cap < 1) return PLX_ERR_INVALID;
    snprintf(buf, (size_t)cap, "splat=%s;blur_axis=%s;slice=%s;vertex_order=%s", L->kn_splat, L->kn_blur, L->kn_slice,
             L->vertex_order ? "morton" : "first_touch");
    return PLX_OK;
}

int64_t plx_block_rows(const plx_lattice *L)
{
    return (L && L->built && L->blocks_ready && L->use_blocks) ? L->n_brows : 0;
}

int plx_prepare(plx_lattice *L, int vd, void *stream)
{
    EntryScope sc(L, stream);
    if (!L) { set_error("plx_prepare: NULL lattice"); return PLX_ERR_INVALID; }
    if (!L->built) { set_error("plx_prepare: lattice not built"); return PLX_ERR_STATE; }
    if (vd < 1) { set_error("plx_prepare: vd = %d must be positive", vd); return PLX_ERR_INVALID; }
    DeviceGuard g(L->device);
    return prepare_tables(L, vd, (hipStream_t)stream);
}

int plx_selftest_sort(int64_t n, int key_bytes, int end_bit, uint64_t seed, void *stream, int64_t *mismatches)
{
    if (n < 1 || n > (1ll << 31) - 8192 || (key_bytes != 4 && key_bytes != 8) || end_bit < 1 || end_bit > 8 * key_bytes || !mismatches) {
        set_error("plx_selftest_sort: n = %lld, %d-byte keys, %d bits", (long long)n, key_bytes, end_bit);
        return PLX_ERR_INVALID;
    }
    return selftest_sort(n, key_bytes, end_bit, seed, (hipStream_t)stream, mismatches);
}

int plx_build_times(const plx_lattice *L, float *h_ms6)
{
    if (!L || !h_ms6) return PLX_ERR_INVALID;
    for (int i = 0; i < 6; ++i) h_ms6[i] = L->build_ms[i];
    return PLX_OK;
}

}  // extern "C"
