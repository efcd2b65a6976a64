/*
 * plx.h -- C ABI of the MI355X permutohedral-lattice filter (libplx.so).
 *
 * This is the drop-in boundary for the reference's one native entry point,
 *
 *     filter(src[N,vd], ref[N,d], coeffs[R]) -> out[N,vd]
 *         gpytorch_lattice_kernel/cpp/lattice.cpp:6-16            (CPU)
 *         gpytorch_lattice_kernel/cuda/permutohedral_cuda.cpp:12-22 (CUDA)
 *
 * restated as plain pointers and sizes (no torch types), plus the staged form
 * the reference fuses into that call (PermutohedralLattice ctor + splat, blur,
 * slice: cpp/permutohedral.h:346-392, 395-486, 513-572, 497-510), so that one
 * lattice can serve every MVM on the same inputs (all conjugate-gradient
 * iterations, the backward pass) and so that a sharded job can put one RCCL
 * all-reduce between splat and blur.
 *
 * Conventions
 *   - every data pointer is DEVICE memory (fp32, row-major, contiguous) on the
 *     lattice's device unless the name starts with h_ (host);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued on it.  A build waits on the host for a few small counts (coordinate ranges, the vertex
 *     count m that sizes the lattice, ...): each arrives through a pinned mailbox the host spins on, the stream
 *     itself is not synchronised.  plx_splat / plx_blur / plx_slice / plx_apply never synchronise and never
 *     allocate once the lattice's tables exist (plx_prepare, or the first MVM of that width) and their workspace
 *     has reached its high-water mark, so they are graph-capturable from then on.  Buffers grow stream-ordered
 *     (hipMallocAsync) on the stream of the call that needs them; a lattice may move between streams as long as
 *     the caller orders the calls;
 *   - every function returns PLX_OK (0) or an error code; nothing calls exit()
 *     (reference: cuda/permutohedral_cuda_kernel.cu:24-32 does).
 *     plx_last_error() returns a thread-local detail string;
 *   - a plx_lattice is not safe for concurrent use from two threads; different lattices may be used from
 *     different threads at the same time (the library keeps no other mutable state than the plx_tune defaults).
 */
#ifndef PLX_H
#define PLX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plx_lattice plx_lattice;

enum {
    PLX_OK = 0,
    PLX_ERR_INVALID = 1,     /* bad argument (shape, NULL, even tap count, ...)        */
    PLX_ERR_HIP = 2,         /* a HIP runtime call failed (see plx_last_error)         */
    PLX_ERR_KEY_RANGE = 3,   /* a lattice coordinate left the int16 key range
                                (the reference wraps silently, permutohedral.h:417-419) */
    PLX_ERR_DIM = 4,         /* d or order outside the compiled range                  */
    PLX_ERR_STATE = 5,       /* lattice not built / wrong sizes for this lattice        */
    PLX_ERR_TOO_LARGE = 6    /* n*(d+1) does not fit the 31-bit entry index             */
};

#define PLX_MAX_DIM 32       /* position dimension d, 1..PLX_MAX_DIM                    */
#define PLX_MAX_ORDER 8      /* taps R = 2*order+1, order 0..PLX_MAX_ORDER              */

/* names for plx_export() */
enum {
    PLX_ARRAY_KEYS = 0,          /* int16  [m][d]        vertex keys, first-touch order (h:73-79)   */
    PLX_ARRAY_ENTRY_VERTEX = 1,  /* int32  [d+1][n]      vertex id of simplex corner r of point p   */
    PLX_ARRAY_ENTRY_WEIGHT = 2,  /* float  [d+1][n]      barycentric weight (h:460-465)             */
    PLX_ARRAY_NEIGHBORS = 3,     /* int32  [d+1][2r][m]  blur neighbour ids, -1 absent (h:539-544)  */
    PLX_ARRAY_ROW_PTR = 4,       /* int32  [m+1]         splat CSR row pointers (owned points)      */
    PLX_ARRAY_CSR_POINT = 5,     /* int32  [nnz]         splat CSR point index                      */
    PLX_ARRAY_CSR_WEIGHT = 6,    /* float  [nnz]         splat CSR weight                           */
    PLX_ARRAY_POINT_PERM = 7     /* uint32 [n]           caller's row of the i-th point in lattice order;
                                    ENTRY_* and CSR_POINT are indexed in lattice order             */
};

const char *plx_strerror(int code);
const char *plx_last_error(void);
/* "libplx <version> gfx950" -- lets a host check which build it loaded */
const char *plx_version(void);

/* A lattice object owns its device buffers (grow-only); re-building it for new
 * inputs reuses them.  `device` is a HIP device ordinal. */
int plx_create(int device, plx_lattice **out);
void plx_destroy(plx_lattice *lat);

/*
 * Build the lattice structure for positions d_ref[n][d] (already divided by the
 * lengthscale, bilateral_kernel.py:198) and stencil taps h_taps[ntaps]
 * (ntaps odd; they set the embedding scale through variance(), h:203-219,
 * h:372-390, and are the blur weights, h:546).
 *
 * Replaces: PermutohedralLattice ctor (h:346-392), the structural half of
 * splat() (h:395-475, 482-484: embedding, hashed vertex creation, replay
 * entries), and every hashTable.lookup() of blur() (h:541-545), which becomes a
 * neighbour table.
 *
 * Internally the points are visited in "lattice order" (shard by shard, inside a
 * shard lexicographically by their rounded lattice coordinates) so that points
 * sharing simplices are adjacent in memory; vertex ids are the reference's
 * first-touch numbering (h:73-79) applied to that order.  The order is an
 * implementation detail: d_src / d_out rows are always in the caller's order.
 *
 * Sharded jobs: the n rows are split into n_shards contiguous near-equal blocks
 * (the first n % n_shards blocks have one extra row); this process splats and
 * slices block `shard_index` only.  Every rank passes the SAME d_ref and
 * n_shards and obtains the same vertex numbering without communication.  A single
 * GPU uses shard_index = 0, n_shards = 1.
 */
int plx_build(plx_lattice *lat, const float *d_ref, int64_t n, int d,
              const float *h_taps, int ntaps,
              int shard_index, int n_shards, void *stream);

/*
 * Sharded build without replicated work (alternative to calling plx_build with the
 * full d_ref on every rank): every rank passes ONLY ITS OWN rows.
 *   1. plx_build_local     embeds / inserts / numbers the rank's own points;
 *   2. the caller exchanges the per-rank vertex keys: m_r = plx_local_vertices(),
 *      keys = [m_r][plx_key_words(d)] uint32 (plx_copy_local_keys), all-gathered in
 *      rank order (RCCL all_gather through torch.distributed in this repo);
 *   3. plx_build_merge     numbers the union (first occurrence in rank order, then
 *      local order -- or along the Morton curve of the vertices, see "vertex_order": either way
 *      the same ids plx_build's shard-major numbering produces),
 *      relabels the local corners, builds the neighbour table over the union and the
 *      splat CSR / slice tables over the rank's rows.
 * Afterwards the lattice behaves like one built by plx_build for that shard:
 * plx_num_points / plx_num_owned = n_local, plx_num_vertices = size of the union.
 */
int plx_build_local(plx_lattice *lat, const float *d_ref_local, int64_t n_local, int d,
                    const float *h_taps, int ntaps, void *stream);
int plx_key_words(int d);                               /* uint32 words per packed vertex key: ceil(d/2) */
int64_t plx_local_vertices(const plx_lattice *lat);     /* m_r after plx_build_local                     */
int plx_copy_local_keys(plx_lattice *lat, void *d_dst, void *stream);   /* d_dst: [m_r][key_words] uint32 */
int plx_build_merge(plx_lattice *lat, const void *d_all_keys, const int64_t *h_counts, int n_ranks,
                    int my_rank, int64_t total_points, void *stream);
/* total_points: points of ALL ranks together (the row counts ride along with the key counts), the same value on every
 * rank; it only feeds the choice of vertex numbering ("vertex_order" under plx_tune), which must fall the same way on
 * every rank.  <= 0: unknown, the choice is made from the key counts alone. */

int64_t plx_num_points(const plx_lattice *lat);    /* n                              */
int64_t plx_num_owned(const plx_lattice *lat);     /* rows of this shard             */
int64_t plx_num_vertices(const plx_lattice *lat);  /* m = hashTable.size(), h:44     */
/* plx_tune("reference_growth", 1) -- LITERAL parity with the reference CPU path where its hash table doubles.  lookup()
 * (cpp/permutohedral.h:104-106) hashes with the capacity in force before lookupOffset() (:58-63) grows the table, so the one
 * lookup that triggers each doubling probes from a stale bucket: a duplicate entry for a key that exists, or a key that
 * later lookups do not find; grow() (:125-161) then re-places entries in old-position order.  The default build is the
 * duplicate-free lattice (which is also what the reference's CUDA path builds: its table never grows).  With the switch
 * on, plx_build / plx_filter replay the reference's table LAYOUT on the host (entry positions only; the EVENTS that shape it
 * -- the m first-touch creations, the stale probe behind each doubling, every lookup of the few keys such a probe touched:
 * O(m) host work, 45-60 ms at N = 1e6, d = 8, m = 1.7e6; value 2 = all N (d+1) lookups one by one, the checker of the
 * event form, 250 ms there) and patch the built structure so that every MVM equals the reference's filter(): the splat
 * contributions the reference loses are dropped, keys its blur-time lookups cannot find read as absent.  Plain
 * single-process builds only (ignored by plx_build_local / plx_build_merge).  h_out6 = {replayed (0/1), entries the
 * reference's table holds (= plx_num_vertices when nothing was replayed or nothing went wrong), dropped (point, corner)
 * contributions, invisible vertices, blur-time missed neighbour (0/1), inexact (0/1: a combination the patched structure
 * cannot express -- never observed)}. */
int plx_reference_growth_info(const plx_lattice *lat, int64_t *h_out6);
int plx_dim(const plx_lattice *lat);               /* d                              */
int plx_order(const plx_lattice *lat);             /* (ntaps-1)/2                    */
/* Row order of d_src / d_out for plx_splat / plx_slice / plx_apply on this lattice:
 * 0 (default) the caller's order -- rows are permuted into lattice order on the way
 * in and back on the way out; 1 the rows ARE in lattice order (row i of this shard
 * = caller row PLX_ARRAY_POINT_PERM[own_begin + i] - own_begin), no permutation
 * work per MVM.  A CG solve permutes its right-hand side once, iterates in
 * lattice order and permutes the solution back once. */
int plx_set_row_order(plx_lattice *lat, int lattice_order);

/* Warm start of the point order (round 6).  on != 0: the NEXT plx_build on this lattice keeps the lattice order of its
 * points from the previous build instead of computing it (coordinate ranges + read-back, sort keys, four radix passes:
 * 0.15 ms of a 1.8 ms build at N = 1e6, d = 8).  For a caller who KNOWS that the positions are the previous build's,
 * re-scaled a little -- a GP training loop whose lengthscale moved: the order is a locality device only (which points sit
 * next to each other in memory), no vertex, weight or neighbour depends on it, so the result is the cold build's up to
 * the order of the fp32 sums inside a vertex row; an order computed for other positions would merely be a slow one.
 * One shot (cleared by the build); ignored unless the row count, dimension and shard are those of the order at hand.
 * plx_order_age: builds since the order was computed from the positions themselves (0 = by the last build, -1 = none). */
int plx_set_reuse_order(plx_lattice *lat, int on);
int plx_order_age(const plx_lattice *lat);

/* Floats per vertex row of a values buffer for vd value columns: 1 for vd = 1,
 * otherwise vd rounded up to a multiple of 4 (rows are whole 16-byte vectors;
 * the padding columns hold zeros).  d_values / d_scratch below are [m][stride]. */
int plx_values_stride(int vd);
/* bytes of device memory currently held by the lattice */
int64_t plx_device_bytes(const plx_lattice *lat);

/*
 * Stage 1 -- splat (h:478-479): d_values[m][stride] = S^T d_src, where d_src holds
 * this shard's rows only, [plx_num_owned][vd], in the caller's row order.  Every row of d_values is
 * written (vertices no owned point touches get 0).  Deterministic: no float
 * atomics.
 */
int plx_splat(plx_lattice *lat, const float *d_src, int vd, float *d_values, void *stream);

/* plx_splat of nb one-hot columns without streaming the corners: column b (< nb <= vd) of d_values is S^T e_p for
 * p = d_points[b], a point index in LATTICE order (device int32; PLX_ARRAY_POINT_PERM maps it to the caller's row); the
 * other columns and rows are zero.  What a pivoted Cholesky of the operator asks for: rows of K = slice(blur(this)).
 * Single-shard lattices. */
int plx_splat_onehot(plx_lattice *lat, const int32_t *d_points, int nb, int vd, float *d_values, void *stream);
/* The whole filter of nb <= 16 one-hot columns: d_out [n][vd] (rows as plx_set_row_order says) = K [e_p0 .. e_p(nb-1) 0 ..],
 * p_b = d_points[b] in LATTICE order as above -- plx_splat_onehot + plx_blur + plx_slice in one call.  sparse != 0: the
 * three stages run on the FRONTIER of the columns' non-zero vertex rows (d + 1 rows per column after the splat, at most
 * 2 r + 1 times as many after every blur axis) instead of streaming all m rows d + 1 times; same operations in the same
 * order as the dense kernels, so the same numbers.  The frontier path needs vd == 1 or vd % 4 == 0 with a 16-byte
 * aligned d_out and a lattice built without "reference_growth"; otherwise (and with sparse == 0) the call runs the three
 * dense stages.  d_values / d_scratch: [m][plx_values_stride(vd)] each, distinct, clobbered.  *d_frontier (device int32,
 * optional): vertex rows the last blur axis worked on (m for the dense stages) -- a caller that batches such calls reads
 * it back to see when the frontier stops being small.  Single-shard lattices. */
int plx_filter_onehot(plx_lattice *lat, const int32_t *d_points, int nb, int vd, float *d_values, float *d_scratch,
                      float *d_out, int sparse, int32_t *d_frontier, void *stream);

/*
 * Stage 2 -- blur (h:513-572): d+1 Jacobi passes over the neighbour table,
 * ping-ponging between d_values and d_scratch (both [m][stride]).  On return
 * *result_in_scratch tells which of the two holds the result (d+1 odd => 1).
 */
int plx_blur(plx_lattice *lat, float *d_values, float *d_scratch, int vd,
             int *result_in_scratch, void *stream);

/*
 * Stage 3 -- slice (h:497-510): d_out[plx_num_owned][vd] = S d_values / (1 + 2^-d)
 * for this shard's rows, in the caller's row order.
 */
int plx_slice(plx_lattice *lat, const float *d_values, int vd, float *d_out, void *stream);

/* splat -> blur -> slice on the lattice's own workspace (single-GPU MVM). */
int plx_apply(plx_lattice *lat, const float *d_src, int vd, float *d_out, void *stream);

/*
 * The rectangular product K(A, B) v -- splat and slice by ROW RANGE (libplx 0.9.1).  Prediction applies the operator
 * between two different point sets (RectangularLazyLattice, bilateral_kernel.py:142-160: K(x*, X) alpha); the reference
 * pads the right-hand side with zeros over the stacked points [X; x*], filters all of them and throws the rows of X away.
 * Here the lattice is still built over the stacked points, and these calls splat only the rows that carry a right-hand
 * side and slice only the rows that are wanted:
 *   plx_splat_rows  d_values[m][stride] = S^T restricted to the caller's rows [row_begin, row_begin + row_count): d_src is
 *                   [row_count][vd].  Every row of d_values is written (vertices no such point touches get 0).
 *   plx_slice_rows  d_out[row_count][vd] = rows [row_begin, row_begin + row_count) of S d_values / (1 + 2^-d).
 *   plx_apply_rows  splat_rows -> plx_blur -> slice_rows on the lattice's own workspace:
 *                   d_out[out_count][vd] = K[out rows, src rows] d_src[src_count][vd],
 * i.e. rows [out_begin, out_begin + out_count) of plx_apply applied to the n-row matrix that holds d_src in rows
 * [src_begin, src_begin + src_count) and zeros elsewhere.  The two ranges are independent (disjoint, equal, nested,
 * overlapping); the full range on both ends is plx_apply.  Swapping them is the transpose, K(B, A) g: the gradient of
 * the product with respect to its right-hand side.
 * Rows are ALWAYS in the caller's order, whatever plx_set_row_order says.  d_src / d_out need 4-byte alignment only;
 * d_values is 16-byte aligned when vd > 1 (PLX_ERR_INVALID otherwise).
 * Lattices built by plain plx_build (or plx_filter) over n points as a single shard: a sharded or merged lattice, and a
 * build that replayed "reference_growth", return PLX_ERR_STATE.  Every argument is checked before any GPU work: NULL
 * pointers, vd < 1, row_count < 1, a range outside [0, n) are PLX_ERR_INVALID; the 2^31 element limits of plx_apply hold
 * for m * stride and row_count * stride (PLX_ERR_TOO_LARGE).
 * Deterministic: no float atomics; two calls with the same arguments are bit-equal.
 * Tables: what a range needs (the vertex-sorted corners of its rows, a stable compaction of the splat CSR; the lattice
 * positions of its rows, ascending) is built by the first call that uses that (row_begin, row_count), on that call's
 * stream, without any read-back, and kept until the lattice's next build; four ranges are kept at once (a product and its
 * transpose alternate on the same lattice), the least recently used one is recycled.  From the second call with the same
 * range and width on, a rows call neither allocates nor synchronises (plx_device_bytes does not move) and is
 * graph-capturable; under stream capture a call that would have to build a table returns PLX_ERR_STATE.
 * plx_last_rows_kernels: "splat=...;slice=..." of the last rows call on this lattice (plx_last_kernels goes on naming
 * the square stages; the blur inside plx_apply_rows reports there).
 */
int plx_splat_rows(plx_lattice *lat, const float *d_src, int64_t row_begin, int64_t row_count, int vd,
                   float *d_values, void *stream);
int plx_slice_rows(plx_lattice *lat, const float *d_values, int vd, int64_t row_begin, int64_t row_count,
                   float *d_out, void *stream);
int plx_apply_rows(plx_lattice *lat, const float *d_src, int64_t src_begin, int64_t src_count, int vd,
                   float *d_out, int64_t out_begin, int64_t out_count, void *stream);
int plx_last_rows_kernels(const plx_lattice *lat, char *buf, int cap);

/*
 * The float64 product (callers detect it by symbol; the version string is unchanged).  The operator is the one plx_apply
 * applies, carried in double: the vertex ids, the neighbour table, the fp32 barycentric weights and the fp32 taps of the
 * build, each converted exactly to double, every sum in double, the result divided by 1 + 2^-d in double.  The lattice
 * itself is the fp32 build's -- positions that a caller holds in double are rounded to float for plx_build, so one build
 * serves both precisions.  What double buys is an accurately APPLIED operator (solves that converge below the 1e-7 at
 * which fp32 products stall), not a more accurate embedding: the lattice approximates the exact kernel to 0.07-0.57
 * relative error either way.  The operator is neither symmetric nor positive (the d + 1 blur passes do not commute), in
 * either precision.
 *   plx_values_stride_f64  doubles per vertex row: 1 for vd = 1, otherwise vd rounded up to a multiple of 2 (rows are
 *                          whole 16-byte vectors); -1 for vd < 1.  d_values / d_scratch below are [m][stride].
 *   plx_splat_f64 / plx_blur_f64 / plx_slice_f64  the three stages on caller buffers of doubles, as plx_splat / plx_blur /
 *                          plx_slice; d_values and d_scratch are distinct and, for vd > 1, 16-byte aligned.
 *   plx_apply_f64          splat -> blur -> slice on a float64 workspace of the lattice: two value planes of doubles,
 *                          allocated by the first fp64 call of a width (fp32 use never allocates them).
 *   plx_last_f64_kernels   "splat=...;blur_axis=...;slice=..." of the last fp64 call (plx_last_kernels goes on naming the
 *                          fp32 stages only).
 * Rows of d_src [n][vd] and d_out [n][vd] are ALWAYS in the caller's order, whatever plx_set_row_order says; they need
 * 8-byte alignment only.  Scope and refusals are those of plx_apply_rows: plain single-shard builds (plx_build or
 * plx_filter); a sharded or merged lattice and a build that replayed "reference_growth" return PLX_ERR_STATE.  Every
 * argument is checked before any GPU work: NULL pointers, vd < 1, misaligned buffers are PLX_ERR_INVALID; m * stride and
 * n * stride stay under 2^31 elements (PLX_ERR_TOO_LARGE).
 * Deterministic: the splat gathers by vertex over the vertex-sorted corners in order, no float atomics; two calls with the
 * same arguments are bit-equal, and the staged calls give the bits of plx_apply_f64.
 * The first fp64 splat after a build makes the vertex-sorted corner table and its row pointer (no read-back), and the
 * first plx_apply_f64 of a width grows the workspace; under stream capture such a call returns PLX_ERR_STATE.  Later
 * calls neither allocate nor synchronise (plx_device_bytes does not move) and are graph-capturable.
 */
int plx_values_stride_f64(int vd);
int plx_splat_f64(plx_lattice *lat, const double *d_src, int vd, double *d_values, void *stream);
int plx_blur_f64(plx_lattice *lat, double *d_values, double *d_scratch, int vd, int *result_in_scratch, void *stream);
int plx_slice_f64(plx_lattice *lat, const double *d_values, int vd, double *d_out, void *stream);
int plx_apply_f64(plx_lattice *lat, const double *d_src, int vd, double *d_out, void *stream);
int plx_last_f64_kernels(const plx_lattice *lat, char *buf, int cap);

/*
 * The float64 rectangular product K(A, B) v by row range (callers detect it by symbol; the version string is unchanged):
 * plx_splat_rows / plx_slice_rows / plx_apply_rows with the arithmetic of the float64 product -- the fp32 weights and taps
 * converted exactly, every sum in double, one division by 1 + 2^-d in double.
 *   plx_splat_rows_f64  d_values[m][plx_values_stride_f64(vd)] = S^T restricted to the caller's rows [row_begin, row_begin +
 *                       row_count): d_src is [row_count][vd].  Every vertex row is written (vertices the range does not
 *                       touch get 0); there is no zero-fill pass.
 *   plx_slice_rows_f64  d_out[row_count][vd] = rows [row_begin, row_begin + row_count) of S d_values / (1 + 2^-d).
 *   plx_apply_rows_f64  splat_rows_f64 -> the blur of plx_apply_f64 -> slice_rows_f64 on the float64 workspace that
 *                       plx_apply_f64 owns (the same two value planes, no second workspace).
 *   plx_last_rows_f64_kernels  "splat=...;slice=..." of the last fp64 rows call (the blur inside plx_apply_rows_f64 reports
 *                       through plx_last_f64_kernels).
 * Rows are ALWAYS in the caller's order.  d_src / d_out need 8-byte alignment only; d_values is 16-byte aligned when
 * vd > 1 (PLX_ERR_INVALID otherwise).
 * Scope and refusals are those of plx_apply_rows and plx_apply_f64 together: a lattice that is not built, a sharded or
 * merged lattice and a build that replayed "reference_growth" return PLX_ERR_STATE; NULL pointers, vd < 1, a count < 1, a
 * range outside [0, n), misaligned buffers are PLX_ERR_INVALID; m * stride and row_count * stride stay under 2^31 elements
 * (PLX_ERR_TOO_LARGE).  Every argument is checked before any GPU work.
 * Tables: the range tables are those of the fp32 rows calls -- they hold no values.  The four slots and their least-
 * recently-used recycling are shared between the precisions: a range that an fp32 call built serves the fp64 call, and the
 * reverse.  Under stream capture a call that would have to build a range table or grow the workspace returns
 * PLX_ERR_STATE; from the second call of a (range, width) on, a call neither allocates nor synchronises (plx_device_bytes
 * does not move) and is graph-capturable.
 * Bit contract: every sum is taken in the order of plx_apply_f64 (a range's corners are a stable compaction of the vertex-
 * sorted corners; a dropped term is fma(w, 0, acc) = acc), so for every pair of ranges plx_apply_rows_f64 equals AS VALUES
 * (-0.0 counted equal to +0.0) rows [out_begin, out_begin + out_count) of plx_apply_f64 applied to the n-row matrix that
 * holds d_src in the source rows and zeros elsewhere; the full range on both ends equals plx_apply_f64 in the same way, and
 * the staged calls give the bits of plx_apply_rows_f64.  No float atomics: two calls with the same arguments are bit-equal.
 */
int plx_splat_rows_f64(plx_lattice *lat, const double *d_src, int64_t row_begin, int64_t row_count, int vd,
                       double *d_values, void *stream);
int plx_slice_rows_f64(plx_lattice *lat, const double *d_values, int vd, int64_t row_begin, int64_t row_count,
                       double *d_out, void *stream);
int plx_apply_rows_f64(plx_lattice *lat, const double *d_src, int64_t src_begin, int64_t src_count, int vd,
                       double *d_out, int64_t out_begin, int64_t out_count, void *stream);
int plx_last_rows_f64_kernels(const plx_lattice *lat, char *buf, int cap);   /* "splat=...;slice=..." */

/*
 * The float64 conjugate-gradient solve on the float64 product (callers detect it by symbol; the version string is
 * unchanged): the vector work of a batched CG iteration and the (s K + sigma^2 I) v of a GP solve, in double.
 *   plx_coldot_f64             d_out[c] = sum_r a[r][c] b[r][c]; d_work: plx_coldot_work_doubles(vd) doubles (-1 for a vd
 *                              outside 1..256; monotone inside).
 *   plx_cg_step_update_f64     alpha = active ? rs / max(pAp, 1e-300) : 0;  X += alpha P;  R -= alpha AP;  rs_new = |R|^2
 *                              (d_work as for plx_coldot_f64).
 *   plx_cg_step_direction_f64  beta = active ? rs_new / max(rs, 1e-300) : 0;  P = R + beta P;
 *                              active_out = active and sqrt(rs_new) / b_norm > tol     (active_out != active).
 * These are plx_coldot / plx_cg_step_update / plx_cg_step_direction with EVERY array in double (row-major [n][vd] matrices;
 * alpha, beta, rs, pAp, b_norm and active -- 1.0 / 0.0 -- double [vd]).  The guard is 1e-300 instead of the fp32 calls'
 * 1e-30: a double solve of a right-hand side scaled by 1e-20 has pAp near 1e-40, which the fp32 guard would silently turn
 * into a wrong alpha.  1 <= vd <= 256, n >= 1.  Deterministic: partial sums per workgroup, then a fixed-order final sum; no
 * float atomics; two calls with the same arguments are bit-equal.  They never allocate and never synchronise, so they
 * are graph-capturable.  Every argument is checked before any launch: a NULL pointer, a vd outside the range, n < 1, a
 * pointer that is not 8-byte aligned and d_active_out == d_active are PLX_ERR_INVALID.
 *   plx_apply_affine_f64       d_out = a * (K d_src) + b * d_src with (a, b) = d_scale_shift[0..1], two doubles read on the
 *                              device.  K d_src is the value plx_apply_f64 gives (its splat and blur run unchanged on the
 *                              same workspace; the slice has the tail fused); out = fma(a, y, b * x) per element.  Rows in the
 *                              caller's order, as for every fp64 call.  Scope, refusals, workspace and the capture rule are
 *                              those of plx_apply_f64; in addition d_out must not alias d_src (PLX_ERR_INVALID).
 *                              d_dot (optional): d_dot[c] = <d_src[:, c], d_out[:, c]> for c < vd, from the slice kernel's
 *                              registers -- one partial row per workgroup in d_work, in a fixed order, then the final
 *                              stage of plx_coldot_f64.  Served for vd <= 128 (rows of up to 64 chunks); d_dot != NULL with
 *                              vd > 128 is PLX_ERR_INVALID: pass NULL and call plx_coldot_f64.
 *   plx_affine_dot_work_doubles  doubles of d_work for that d_dot; -1 where the dot is not served or the lattice is not
 *                              built.  With d_dot == NULL, d_work may be NULL.
 * The slice reports through plx_last_f64_kernels, in the slice field (f64_affine_v1_kernel / f64_affine_chunk_kernel /
 * f64_affine_wide_kernel, gated like the slices of plx_apply_f64).
 * Two exactness contracts: (i) with (a, b) = (1, 0) d_out equals plx_apply_f64 AS VALUES (-0.0 counted equal to +0.0; finite
 * d_src): the sums are formed from the same pieces in the same order and the tail adds 0.  (ii) d_dot and
 * plx_coldot_f64(d_src, d_out) agree to (n + 4) 2^-52 of sum_r |src out| each, not to the bit: their partial sums are cut
 * differently (by workgroups of lattice-ordered points there, by ranges of caller rows here).
 */
int64_t plx_coldot_work_doubles(int vd);
int plx_coldot_f64(const double *d_a, const double *d_b, int64_t n, int vd, double *d_out, double *d_work, void *stream);
int plx_cg_step_update_f64(double *d_x, double *d_r, const double *d_p, const double *d_ap, const double *d_rs,
                           const double *d_pap, const double *d_active, int64_t n, int vd, double *d_rs_new,
                           double *d_alpha, double *d_work, void *stream);
int plx_cg_step_direction_f64(double *d_p, const double *d_r, const double *d_rs_new, const double *d_rs,
                              const double *d_active, const double *d_b_norm, double tol, int64_t n, int vd,
                              double *d_beta, double *d_active_out, void *stream);
int64_t plx_affine_dot_work_doubles(const plx_lattice *lat, int vd);
int plx_apply_affine_f64(plx_lattice *lat, const double *d_src, int vd, double *d_out, const double *d_scale_shift,
                         double *d_dot, double *d_work, void *stream);

/*
 * The transposed and the symmetrised float64 products (callers detect them by symbol; the version string is unchanged).
 * K = S B_d ... B_0 S^T / (1 + 2^-d) is not symmetric.  On a plain build the neighbour table is symmetric, so the
 * transpose of one axis blur is that axis with mirrored taps (c'[i] = c[2 r - i]) and K^T runs the axes d .. 0 with them.
 * K_s = (K + K^T) / 2 is symmetric to rounding; it is NOT proven positive (its smallest eigenvalue was -0.016 against a
 * largest of 378 on one measured lattice), but plain CG converges on K_s + noise I at noise levels where it stalls on K.
 *   plx_blur_t_f64        the adjoint of plx_blur_f64, with its arguments: the kernels of plx_blur_f64, host code only.
 *   plx_apply_t_f64       splat -> blur_t -> slice: K^T d_src, on the workspace of plx_apply_f64.
 *   plx_blur_sym_f64      0.5 (blur(values) + blur_t(values)) in d + 1 launches, each advancing both chains
 *                         (reported as f64_blur_dual_kernel; a profiler shows blur_dual_kernel<double, ...>, the double
 *                         instance of the template the fp32 form below shares, csrc/plx_sym_kernels.h): launch k takes the
 *                         forward chain through axis k, the reverse chain through axis d - k; the first reads the one input
 *                         plane for both, the last stores the one mean.
 *                         d_work: plx_blur_sym_work_doubles(lat, vd) doubles (min(d + 1, 3) planes of m * stride; -1 for
 *                         vd < 1 or an unbuilt lattice), 16-byte aligned for vd > 1, not overlapping d_values.  *d_result
 *                         is set on the host, without synchronisation, to d_values or to a plane of d_work: where the
 *                         result lies.  d_values is clobbered.
 *   plx_apply_sym_f64     splat -> blur_sym -> slice: K_s d_src.  Runs on the workspace of plx_apply_f64 and two further
 *                         planes that the first such call of a width allocates.
 *   plx_apply_affine_sym_f64  plx_apply_affine_f64 with K_s for K: d_out = a K_s d_src + b d_src, the same arguments, the
 *                         same affine slice kernels for the tail and d_dot (plx_affine_dot_work_doubles).
 *   plx_last_sym_f64_kernels  "splat=...;blur=...;slice=..." of the last transposed or symmetrised call.  These calls leave
 *                         what plx_last_f64_kernels reports untouched.
 * Scope, refusals, alignment, the 2^31 limits and the capture rule are those of plx_apply_f64; a build that replayed
 * "reference_growth" returns PLX_ERR_STATE because its neighbour table is not symmetric, so the reverse-axes identity does
 * not hold there.  After the first call of a width, no call allocates or synchronises.
 * Bit contracts: each chain's sums are formed as plx_blur_f64 forms them (same slots, same order, same fmas), the mean is
 * one rounded sum and an exact halving, so plx_blur_sym_f64 gives the bits of 0.5 * (plx_blur_f64 + plx_blur_t_f64) formed
 * in double by the caller; the staged calls give the bits of plx_apply_t_f64 and plx_apply_sym_f64; with (a, b) = (1, 0)
 * plx_apply_affine_sym_f64 equals plx_apply_sym_f64 as values.  No atomics: two calls with the same arguments are bit-equal.
 */
int plx_blur_t_f64(plx_lattice *lat, double *d_values, double *d_scratch, int vd, int *result_in_scratch, void *stream);
int plx_apply_t_f64(plx_lattice *lat, const double *d_src, int vd, double *d_out, void *stream);
int64_t plx_blur_sym_work_doubles(const plx_lattice *lat, int vd);
int plx_blur_sym_f64(plx_lattice *lat, double *d_values, double *d_work, int vd, double **d_result, void *stream);
int plx_apply_sym_f64(plx_lattice *lat, const double *d_src, int vd, double *d_out, void *stream);
int plx_apply_affine_sym_f64(plx_lattice *lat, const double *d_src, int vd, double *d_out, const double *d_scale_shift,
                             double *d_dot, double *d_work, void *stream);
int plx_last_sym_f64_kernels(const plx_lattice *lat, char *buf, int cap);

/*
 * The transposed and the symmetrised fp32 products (callers detect them by symbol; the version string is unchanged): the
 * block above in the precision of plx_apply.  The plain fp32 blur picks among ten kernel families, some with two axes per
 * launch; these calls run ONE family whatever the shape:
 *   plx_blur_t            axes d .. 0 with mirrored taps, one launch of blur_axis_kernel (the general family of plx_blur)
 *                         per axis: host code only.  Arguments of plx_blur; d_values and d_scratch must not overlap and are
 *                         16-byte aligned for vd > 1.
 *   plx_apply_t           splat -> blur_t -> slice: K^T d_src, on the workspace of plx_apply.
 *   plx_blur_sym          0.5 (blur(values) + blur_t(values)) in d + 1 launches of blur_dual_kernel, each advancing both
 *                         chains on separate planes; the first reads the one input plane for both, the last stores the one
 *                         mean.  d_work: plx_blur_sym_work_floats(lat, vd) floats (min(d + 1, 3) planes of
 *                         m * plx_values_stride(vd); -1 for vd < 1 or an unbuilt lattice), 16-byte aligned for vd > 1, not
 *                         overlapping d_values.  *d_result is set on the host, without synchronisation, to d_values or to
 *                         a plane of d_work: where the result lies.  d_values is clobbered.
 *   plx_apply_sym         splat -> blur_sym -> slice: K_s d_src.  Runs on the workspace of plx_apply and two further
 *                         planes that the first such call of a width allocates (refused under stream capture, PLX_ERR_STATE;
 *                         afterwards no call allocates or synchronises).
 *   plx_apply_affine_sym  plx_apply_affine and plx_apply_affine_dot in one, with K_s for K: d_out = a K_s d_src + b d_src.
 *                         d_work == NULL: the affine tail only.  d_work set (plx_affine_dot_work_floats; vd in 2..256),
 *                         d_dot == NULL: the per-tile partial sums of the column dots <d_src, d_out> stay in d_work, in the
 *                         layout of plx_apply_affine_dot (plx_affine_dot_tiles rows).  Both set: d_dot receives the dots.
 *                         d_out == d_src is PLX_ERR_INVALID.
 *   plx_last_sym_kernels  "splat=...;blur=...;slice=..." of the last such call.  These calls leave what plx_last_kernels
 *                         reports untouched.
 * Rows follow plx_set_row_order exactly as in plx_apply.  Refusals, before any launch: NULL pointers and vd < 1
 * (PLX_ERR_INVALID); an unbuilt lattice, a sharded or merged one, a build that replayed "reference_growth" (its neighbour
 * table is not symmetric) (PLX_ERR_STATE); m * stride or n * stride >= 2^31 (PLX_ERR_TOO_LARGE).
 * Bit contracts: each chain's sums are blur_axis_kernel's (same slots, same order, same expression forms), the mean is one
 * rounded sum and an exact halving: wherever plx_blur itself runs the general family, plx_blur_sym gives the bits of
 * 0.5f * (plx_blur + plx_blur_t) formed by the caller; in the other families the two differ by the rounding of those
 * families.  The staged calls give the bits of plx_apply_t and plx_apply_sym; with (a, b) = (1, 0) plx_apply_affine_sym
 * equals plx_apply_sym as values.  No atomics: two calls with the same arguments are bit-equal.
 * K_s is symmetric to rounding; it is NOT proven positive.
 */
int plx_blur_t(plx_lattice *lat, float *d_values, float *d_scratch, int vd, int *result_in_scratch, void *stream);
int plx_apply_t(plx_lattice *lat, const float *d_src, int vd, float *d_out, void *stream);
int64_t plx_blur_sym_work_floats(const plx_lattice *lat, int vd);
int plx_blur_sym(plx_lattice *lat, float *d_values, float *d_work, int vd, float **d_result, void *stream);
int plx_apply_sym(plx_lattice *lat, const float *d_src, int vd, float *d_out, void *stream);
int plx_apply_affine_sym(plx_lattice *lat, const float *d_src, int vd, float *d_out, const float *d_scale_shift,
                         float *d_dot, float *d_work, void *stream);
int plx_last_sym_kernels(const plx_lattice *lat, char *buf, int cap);

/*
 * The true diagonal of the operator (callers detect it by symbol; the version string is unchanged): K_ii of
 * K = S B_d ... B_0 S^T / (1 + 2^-d), per point, exactly the sum the product forms -- not the unit diagonal the kernel
 * classes declare.  With the corners v_a and the weights w_a of point i,
 *     K_ii = (1 / (1 + 2^-d)) sum_{a,b} w_a w_b (B_d ... B_0)[v_a, v_b],
 * and an entry of the blur product is a sum of at most 2 r + 1 paths through the neighbour table (one hop per axis, shifts
 * c + s_j with s the 0 / +-1 pattern of the corner pair; csrc/plx_diag_kernels.h).  The taps are the lattice's own, those
 * of its build.  diag(K^T) = diag(K), so the same values are the diagonal of plx_apply_t and of plx_apply_sym.
 *   plx_diag      d_out[i - row_begin] = K_ii for the caller rows row_begin <= i < row_begin + row_count, every sum carried
 *                 in fp32 (4-byte aligned).  On the stacked lattice [xout; xin] of a prediction the range of xin is
 *                 diag K(x*, x*).  lattice_rows != 0: the same values in lattice position order (plx_copy_point_perm), for
 *                 the whole range [0, n) only.  The call takes this flag and ignores plx_set_row_order.
 *   plx_diag_f64  the same with every sum carried in double (the fp32 weights and taps converted exactly; 8-byte aligned).
 * One launch, no workspace, no allocation, no synchronisation: legal under stream capture from the first call on;
 * plx_device_bytes and what plx_last_kernels / plx_last_f64_kernels report are left as they were.  Refusals, all before the
 * launch, the output untouched: a NULL pointer, row_count < 1, a range outside [0, n), lattice_rows with another range than
 * [0, n), a misaligned output (PLX_ERR_INVALID); an unbuilt lattice, a sharded or merged one, a build that replayed
 * "reference_growth" (its table is not symmetric and its splat weights differ from its slice weights) (PLX_ERR_STATE).
 * Order 0 goes through the same code: c_0^(d+1) sum_a w_a^2 / (1 + 2^-d).  Every output element is written by one thread
 * from sums in a fixed order, no atomics: two calls are bit-equal.  The fp32 values stay within
 * ((d+1)^2 (2r+1) + d + 4) 2^-24 of the size of the terms they sum, the float64 ones within the same count of 2^-52.
 */
int plx_diag(plx_lattice *lat, int64_t row_begin, int64_t row_count, int lattice_rows, float *d_out, void *stream);
int plx_diag_f64(plx_lattice *lat, int64_t row_begin, int64_t row_count, int lattice_rows, double *d_out, void *stream);

/*
 * Queries at points that are not the build's (callers detect them by symbol; the version string is unchanged): locate
 * foreign points in a built lattice once, then slice any vertex array there, without a new build.  The operator is
 *     K_q(x*, X) = S* B_d ... B_0 S_X^T / (1 + 2^-d),
 * where S* holds a query's barycentric weights on those of its d + 1 simplex corners that are vertices of X's lattice; an
 * absent corner contributes nothing.  It is NOT the stacked operator of plx_apply_rows on [x*; X], whose blur also runs
 * through vertices that exist only because of the query points; how much of a query the lattice supports is data-dependent,
 * which is why plx_locate reports the weight mass it found.
 *   plx_locate    d_x [nq][d] in the units of plx_build's d_ref (already divided by the lengthscale).  d_vid [d+1][nq] int32
 *                 and d_w [d+1][nq] float have the SoA layout of the build's corner tables: d_vid[r][q] is the id of corner r
 *                 in the numbering of the CURRENT build, or -1 when that key is not a vertex; d_w[r][q] is always the
 *                 barycentric weight, with the bits the build gives a point at the same position.  d_mass (may be NULL)
 *                 [nq]: the fp32 sum, in corner order, of the weights of the corners found -- 1 where the whole simplex
 *                 exists.  A query with a coordinate outside the int16 key range, NaN or Inf gets every id -1 and mass 0;
 *                 that is no error and the lattice stays usable.  A location is stale after the next build of `lat`; the
 *                 library cannot know (simplex_gp_amd.lattice.LatticeQuery carries the build id).
 *   plx_slice_at / plx_slice_at_f64
 *                 d_values: a vertex array with row stride plx_values_stride(vd) / plx_values_stride_f64(vd), as plx_splat +
 *                 plx_blur (or their _f64 forms) leave it, in whichever buffer the blur reports; 16-byte aligned for
 *                 vd > 1.  d_out [nq][vd], dense, in query order:
 *                     out[q][c] = sum over r with vid >= 0 of w_r values[vid_r][c] / (1 + 2^-d),
 *                 in the expression forms and corner order of plx_slice_rows / plx_slice_f64: for a query at a build point
 *                 the bits of that point's row of those calls.  An absent corner is skipped, not multiplied by zero.
 *   plx_last_query_kernels  "locate=...;slice_at=...;dots=...;pullback=..." of the last such calls (the last two: below).
 * Each call is one launch: no workspace, no allocation, no read-back, legal under stream capture.  Refusals, all before
 * the launch, the outputs untouched: a NULL pointer (d_mass excepted), nq < 1, vd < 1, a misaligned buffer, an output
 * that aliases an input (PLX_ERR_INVALID); an unbuilt lattice, a sharded or merged one, a build that replayed
 * "reference_growth", the single-use lattice of plx_filter (PLX_ERR_STATE); m * stride or nq * stride >= 2^31
 * (PLX_ERR_TOO_LARGE), the column limit of plx_slice_rows / plx_slice_f64.
 */
int plx_locate(plx_lattice *lat, const float *d_x, int64_t nq, int32_t *d_vid, float *d_w, float *d_mass, void *stream);
int plx_slice_at(plx_lattice *lat, const float *d_values, int vd, const int32_t *d_vid, const float *d_w, int64_t nq,
                 float *d_out, void *stream);
int plx_slice_at_f64(plx_lattice *lat, const double *d_values, int vd, const int32_t *d_vid, const float *d_w, int64_t nq,
                     double *d_out, void *stream);
int plx_last_query_kernels(const plx_lattice *lat, char *buf, int cap);

/*
 * The position gradient of a query (callers detect it by symbol; the version string is unchanged).  plx_slice_at is
 * piecewise linear in the query position: inside the simplex plx_locate chose, the weights are affine in it.  For an
 * upstream gradient d_gout [nq][vd] of plx_slice_at's output, the exact derivative of what the forward computes is two
 * launches with the array d_t [d+1][nq] between them, which the caller supplies:
 *   plx_slice_at_dots / plx_slice_at_dots_f64
 *                 d_t[r][q] = <d_gout[q][:], d_values[d_vid[r][q]][:]> / (1 + 2^-d) for the corners found, exactly 0 for the
 *                 absent ones (no gather: the vertex array may be non-finite elsewhere, and in its stride padding).  The
 *                 derivative with respect to the weight d_w[r][q].  d_values, vd, d_vid as for plx_slice_at.
 *   plx_locate_pullback / plx_locate_pullback_f64
 *                 d_gx[q][j] = s_j (sum_{i <= j} e_i - (j + 1) e_{j+1}),  e_i = (t[d - rk_i] - t[(d + 1 - rk_i) mod (d + 1)]) / (d + 1),
 *                 dense [nq][d], with s the build's scale factors and rk the rank permutation of the embedding, recomputed
 *                 from the SAME d_x plx_locate read (so the simplex is the one it chose).  A query plx_locate rejects
 *                 (out of the key range, NaN, Inf) gets a zero row.  d_t need not come from plx_slice_at_dots: any
 *                 derivative with respect to the weights is pulled back.
 * No atomics; two calls give the same bits.  Gradients with respect to d_values are not computed.  Each call is one launch
 * with no workspace, legal under stream capture, and refuses what plx_slice_at / plx_locate refuse, the outputs untouched;
 * nq * (d + 1) >= 2^31 is PLX_ERR_TOO_LARGE.
 */
int plx_slice_at_dots(plx_lattice *lat, const float *d_values, int vd, const int32_t *d_vid, const float *d_gout, int64_t nq,
                      float *d_t, void *stream);
int plx_slice_at_dots_f64(plx_lattice *lat, const double *d_values, int vd, const int32_t *d_vid, const double *d_gout,
                          int64_t nq, double *d_t, void *stream);
int plx_locate_pullback(plx_lattice *lat, const float *d_x, const float *d_t, int64_t nq, float *d_gx, void *stream);
int plx_locate_pullback_f64(plx_lattice *lat, const float *d_x, const double *d_t, int64_t nq, double *d_gx, void *stream);

/*
 * The splat at query points (callers detect it by symbol; the version string is unchanged): S*^T g, the query twin of
 * plx_splat and the adjoint of plx_slice_at without its 1 / (1 + 2^-d),
 *     values[v][c] = sum over the corners (r, q) with d_vid[r][q] == v of d_w[r][q] g[q][c].
 * With plx_blur_t / plx_blur_t_f64 and plx_slice / plx_slice_f64 after it, it is K_q^T g = K(X, x*) g; the call carries no
 * scaling flag.  Two steps, no atomics:
 *   plx_query_plan_bytes  the bytes a plan of nq queries needs on the current build (a function of m, d and nq alone); -1
 *                 for an unbuilt lattice, nq < 1 or nq * (d + 1) >= 2^31 - 4096.
 *   plx_query_plan  once per located query (d_vid, d_w as plx_locate left them): the nq (d + 1) corner pairs, pair index
 *                 r * nq + q, sorted by vertex with a stable sort; an absent corner (id -1) and an id outside [0, m) sort
 *                 behind every vertex and index nothing.  d_plan: plx_query_plan_bytes bytes, 16-byte aligned, the
 *                 caller's; it holds the sorted tables AND the sort's scratch, so no buffer of the lattice is touched.
 *                 Inside a vertex the corners stand in ascending pair index: that is the summation order of the splat,
 *                 and two plans of one query are equal byte for byte in their tables.
 *   plx_splat_at / plx_splat_at_f64
 *                 d_g [nq][vd], dense; d_values [m][plx_values_stride(vd)] / [m][plx_values_stride_f64(vd)], 16-byte
 *                 aligned for vd > 1.  EVERY row is written: exact zeros at a vertex no query corner lands on and in the
 *                 stride padding.  One launch of the kernels of plx_splat_rows / plx_splat_rows_f64, the family chosen by
 *                 the row width alone; a vertex sums fma(w, g, acc) over its corners in plan order.
 *   plx_last_splat_at_kernels  "plan=...;splat_at=..." of the last such calls.
 * The library CANNOT tell whether a plan was made on this build or for this nq: a plan of another build or another nq
 * is read as if it were right (simplex_gp_amd.query_adjoint.QueryPlan carries both and refuses).  Launches only: no
 * allocation, no read-back, legal under stream capture.  Refusals, all before the first launch, the outputs untouched:
 * those of plx_slice_at, an output that overlaps an input or the plan among them (PLX_ERR_INVALID), and
 * nq * (d + 1) >= 2^31 - 4096, the sort's limit (PLX_ERR_TOO_LARGE).
 */
int64_t plx_query_plan_bytes(const plx_lattice *lat, int64_t nq);
int plx_query_plan(plx_lattice *lat, const int32_t *d_vid, const float *d_w, int64_t nq, void *d_plan, void *stream);
int plx_splat_at(plx_lattice *lat, const void *d_plan, const float *d_g, int vd, int64_t nq, float *d_values, void *stream);
int plx_splat_at_f64(plx_lattice *lat, const void *d_plan, const double *d_g, int vd, int64_t nq, double *d_values,
                     void *stream);
int plx_last_splat_at_kernels(const plx_lattice *lat, char *buf, int cap);

/*
 * The float64 position gradient (callers detect it by symbol; the version string is unchanged): plx_apply_backward with
 * every array in double, for every column count.  `lat` is built with the DERIVATIVE taps on the positions rounded to
 * float, as for every fp64 call; d_x [n][d] is the caller's FLOAT64 position matrix (not the rounded copy), d_g (the
 * incoming gradient) and d_src (the forward right-hand side) are [n][nrhs], all rows in the caller's order.  With
 * L = nrhs and C = 2 L (1 + d) (always even: a value row is L (1 + d) chunks of two doubles), the stacked matrix is
 * [ g | g (x) x | src | src (x) x ], [n][C], the product blocks l-major (column L + l d + k holds g_l x_k).  Neither it
 * nor its filtered image is stored by plx_apply_backward_f64.
 *   plx_backward_splat_f64     d_values[m][C] = the plx_splat_f64 of the stacked matrix, each stack element formed inside
 *                              the splat as ONE rounded double multiply (plain columns are copied) and accumulated as
 *                              fma((double)w, element, acc) in the corner order of plx_splat_f64.  d_values is 16-byte
 *                              aligned.
 *   plx_backward_contract_f64  slice and contraction in one kernel: from d_values (blurred by plx_blur_f64 at vd = C) every
 *                              point's filtered row [ wg | wgx | ws | wsx ] is formed on chip with the sums of
 *                              plx_slice_f64 (one division by 1 + 2^-d) and contracted to
 *                                d_grad_x[row][k] = -2 sum_l ( s_l x_k wg_l - s_l wgx_lk + g_l x_k ws_l - g_l wsx_lk ),  k < d,
 *                              the sum started at 0 and taken for l ascending, the four terms in the order written, the
 *                              products s_l x_k and g_l x_k formed first; unless d_grad_src is NULL,
 *                              d_grad_src[row][l] = wg_l.
 *   plx_apply_backward_f64     the two around the blur of plx_apply_f64, on the float64 workspace that plx_apply_f64 owns;
 *                              the arguments of plx_apply_backward, in double.
 * The kernels report through plx_last_f64_kernels: f64_backward_splat_chunk_kernel / f64_backward_splat_wide_kernel in the
 * splat field, f64_backward_contract_chunk_kernel / f64_backward_contract_wide_kernel in the slice field (the chunk shape
 * up to 64 chunks, i.e. C <= 128; the wide shape above).
 * Column limit: the contraction keeps a point's row on chip, four rows of C doubles in the 64 KiB of LDS of a workgroup,
 * so C <= 2048; above that every call returns PLX_ERR_INVALID before any launch.
 * Scope, refusals, workspace growth and the capture rule are those of plx_apply_f64.  PLX_ERR_STATE: a lattice that is not
 * built, a sharded or merged build, a build that replayed "reference_growth", the first call of a width (or the first fp64
 * splat after a build) under stream capture.  PLX_ERR_INVALID: a NULL pointer other than d_grad_src, nrhs < 1, a pointer
 * off 8-byte alignment, d_values off 16-byte alignment, an output that is an input or the other output.
 * PLX_ERR_TOO_LARGE: m * C or n * C at or over 2^31.  Every argument is checked before any GPU work; from the second call
 * of a width on, a call neither allocates nor synchronises (plx_device_bytes does not move) and is graph-capturable.
 * No float atomics, every output element written by exactly one thread: two calls with the same arguments are bit-equal.
 * Two contracts.  (i) Bits: plx_backward_splat_f64 equals AS VALUES (-0.0 counted equal to +0.0) plx_splat_f64 of the
 * explicit stacked matrix formed in double with one multiply per product element; d_grad_src equals AS VALUES columns
 * [0, L) of plx_apply_f64 of that matrix; the staged calls (splat, plx_blur_f64, contract) give the bits of
 * plx_apply_backward_f64.  (ii) Bar: every entry of d_grad_x is within 2 (k + 4 (L + 1)) 2^-52 of the size of the terms it
 * sums (k: the depth of the fp64 product's sums, tests/test_backward_f64_gpu.py) of the gradient formed from a float64
 * filter of the stack; bit equality with a contraction written in torch is not promised (its sum runs in another order).
 */
int plx_backward_splat_f64(plx_lattice *lat, const double *d_g, const double *d_src, const double *d_x, int nrhs,
                           double *d_values, void *stream);
int plx_backward_contract_f64(plx_lattice *lat, const double *d_values, const double *d_g, const double *d_src,
                              const double *d_x, int nrhs, double *d_grad_x, double *d_grad_src /* may be NULL */,
                              void *stream);
int plx_apply_backward_f64(plx_lattice *lat, const double *d_g, const double *d_src, const double *d_x, int nrhs,
                           double *d_grad_x, double *d_grad_src /* may be NULL */, void *stream);

/*
 * The float64 position gradient of the rectangular product K(A, B) v, one side per call (callers detect it by symbol; the
 * version string is unchanged).  With G the incoming gradient (non-zero on the out rows only) and S the right-hand side
 * (non-zero on the source rows only), the four terms of the square gradient above split: on the source rows only
 * s_l x_k wg_l - s_l wgx_lk lives, on the out rows only g_l x_k ws_l - g_l wsx_lk.  One call serves one side: it filters the
 * HALF stack [ a | a (x) x ] of the rows of a to the rows of b and contracts it there against b.  (a = g on the out rows,
 * b = src on the source rows) gives the gradient of the source rows' positions, (a = src, b = g) that of the out rows'.
 * `lat` is built with the DERIVATIVE taps on the stacked positions rounded to float, as for plx_apply_backward_f64; d_x
 * [n][d] is the caller's FLOAT64 position matrix of ALL stacked points.  L = nrhs, H = L (1 + d) (>= 2),
 * stride = plx_values_stride_f64(H) (H rounded up to even).  The product block is l-major: column L + l d + k holds a_l x_k,
 * x the row a_begin + r of d_x.
 *   plx_backward_splat_rows_f64     d_a is [a_count][L].  d_values[m][stride] = the plx_splat_rows_f64 over rows [a_begin,
 *                                   a_begin + a_count) of the half stack, each product element formed inside the splat as
 *                                   ONE rounded double multiply (plain columns are copied) and accumulated as
 *                                   fma((double)w, element, acc) in the corner order of the range's table.  Every vertex
 *                                   row is written: a vertex the range does not touch gets 0, the padding column of an odd
 *                                   H gets 0; there is no zero-fill pass.
 *   plx_backward_contract_rows_f64  slice and contraction in one kernel: for row i of [b_begin, b_begin + b_count) the
 *                                   filtered row [ wa | wax ] is formed on chip from d_values (blurred by plx_blur_f64 at
 *                                   vd = H) with the sums of plx_slice_rows_f64 (one division by 1 + 2^-d) and contracted to
 *                                     d_grad_x[i][k] = -2 sum_l ( (b_l x_k) wa_l - b_l wax_lk ),  k < d,
 *                                   the sum started at 0 and taken for l ascending, the two terms in the order written,
 *                                   b_l x_k formed first, x the row b_begin + i of d_x.  d_b is [b_count][L], d_grad_x
 *                                   [b_count][d]; unless d_filtered is NULL, d_filtered[i][l] = wa_l, [b_count][L].
 *   plx_apply_backward_rows_f64     the two around the blur of plx_apply_f64 at width H, on the float64 workspace that
 *                                   plx_apply_f64 owns: m x stride doubles per plane, half of what the padded square
 *                                   gradient needs.
 * Rows are ALWAYS in the caller's order.  The two ranges are independent: disjoint, equal, nested or overlapping.  The
 * range tables are the slots of the rows calls, shared with them and across precisions; nothing new is stored per range.
 * The splat and the contraction report through plx_last_rows_f64_kernels (rows64_backward_splat_chunk_kernel /
 * rows64_backward_splat_wide_kernel in the splat field, rows64_backward_contract_chunk_kernel /
 * rows64_backward_contract_wide_kernel in the slice field: the chunk shape up to 64 chunks, i.e. stride <= 128, the wide
 * shape above); the blur reports through plx_last_f64_kernels.  These are the names the library reports; the kernels are the
 * double instances of the templates the fp32 form below shares (csrc/plx_rows_backward_kernels.h), so a profiler shows the
 * symbols rows_backward_splat_chunk_kernel<double> ... rows_backward_contract_wide_kernel<double, D1>.
 * Scope, refusals, workspace growth and the capture rule are those of plx_apply_rows_f64 and plx_apply_backward_f64 together.
 * PLX_ERR_STATE: a lattice that is not built, a sharded or merged build, a build that replayed "reference_growth", and under
 * stream capture a call that would have to build a range table, make the vertex row pointer or grow the workspace.
 * PLX_ERR_INVALID: a NULL pointer other than d_filtered, nrhs < 1, a count < 1, a range outside [0, n), a pointer off 8-byte
 * alignment, d_values off 16-byte alignment, an output that aliases an input or the other output, and stride > 2048 (the
 * wide contraction keeps four rows of `stride` doubles in the 64 KiB of LDS of a workgroup, the limit of
 * plx_apply_backward_f64).  PLX_ERR_TOO_LARGE: m * stride, a_count * stride or b_count * stride at or over 2^31.  Every
 * argument is checked before any GPU work: a refused call writes nothing.  From the second call of a (range pair, width)
 * on, a call neither allocates nor synchronises (plx_device_bytes does not move) and is graph-capturable.  No float
 * atomics, every output element written by exactly one thread: two calls with the same arguments are bit-equal.
 * Two contracts.  (i) Bits, AS VALUES (-0.0 counted equal to +0.0): plx_backward_splat_rows_f64 equals plx_splat_rows_f64
 * of the explicit half stack formed in double with one multiply per product element, in all `stride` columns; d_filtered
 * equals columns [0, L) of plx_apply_rows_f64 of that half stack, and rows [b_begin, b_begin + b_count) of the d_grad_src
 * of plx_apply_backward_f64 on the zero-padded n-row matrices, for every pair of ranges; the staged calls (splat,
 * plx_blur_f64 at vd = H, contract) give the bits of plx_apply_backward_rows_f64.  (ii) Bar: every entry of d_grad_x is
 * within 2 (k + 2 (L + 1)) 2^-52 of the size of the terms it sums (k: the depth of the fp64 product's sums,
 * tests/test_backward_f64_gpu.py) of the contraction of a float64 filter of the half stack, and exactly 0 where no term
 * reaches it.  The two one-sided results added into [n][d] agree with plx_apply_backward_f64 of the padded problem to
 * rounding; bit equality with it is not promised.
 */
int plx_backward_splat_rows_f64(plx_lattice *lat, const double *d_a, int64_t a_begin, int64_t a_count, const double *d_x,
                                int nrhs, double *d_values, void *stream);
int plx_backward_contract_rows_f64(plx_lattice *lat, const double *d_values, const double *d_b, int64_t b_begin,
                                   int64_t b_count, const double *d_x, int nrhs, double *d_grad_x,
                                   double *d_filtered /* may be NULL */, void *stream);
int plx_apply_backward_rows_f64(plx_lattice *lat, const double *d_a, int64_t a_begin, int64_t a_count, const double *d_b,
                                int64_t b_begin, int64_t b_count, const double *d_x, int nrhs, double *d_grad_x,
                                double *d_filtered /* may be NULL */, void *stream);

/*
 * The fp32 position gradient of the rectangular product K(A, B) v, one side per call (callers detect it by symbol; the
 * version string is unchanged): the split of plx_apply_backward_rows_f64 above on buffers of floats.  One call filters the
 * HALF stack [ a | a (x) x ] of the rows of a to the rows of b and contracts it there against b.  (a = g on the out rows,
 * b = src on the source rows) gives the gradient of the source rows' positions, (a = src, b = g) that of the out rows'.
 * `lat` is built with the DERIVATIVE taps on d_x, the [n][d] positions of ALL stacked points.  L = nrhs, H = L (1 + d)
 * (>= 2, so there is no single-column shape), stride = plx_values_stride(H) (H rounded up to 4: value rows are whole
 * float4 chunks).  Column c of the half stack: c < L is the plain column l = c, else the product column
 * (l, k) = divmod(c - L, d), l-major (column L + l d + k holds a_l x_k, x the row a_begin + r of d_x); the padding columns
 * H <= c < stride are 0.
 *   plx_backward_splat_rows     d_a is [a_count][L].  d_values[m][stride] = the plx_splat_rows over rows [a_begin,
 *                               a_begin + a_count) of the half stack, each product element formed inside the splat as ONE
 *                               rounded float multiply (plain columns are copied) and accumulated as acc += w * element in
 *                               the corner order of the range's table.  Every vertex row is written: a vertex the range
 *                               does not touch gets 0; there is no zero-fill pass.
 *   plx_backward_contract_rows  slice and contraction in one kernel: for row i of [b_begin, b_begin + b_count) the filtered
 *                               row [ wa | wax ] is formed on chip from d_values (blurred by plx_blur at vd = H) with the
 *                               sums of plx_slice_rows (every term multiplied by the rounded 1 / (1 + 2^-d)) and contracted to
 *                                 d_grad_x[i][k] = -2 sum_l ( (b_l x_k) wa_l - b_l wax_lk ),  k < d,
 *                               the sum started at 0 and taken for l ascending, the two terms in the order written, b_l x_k
 *                               formed first, x the row b_begin + i of d_x.  d_b is [b_count][L], d_grad_x [b_count][d];
 *                               unless d_filtered is NULL, d_filtered[i][l] = wa_l, [b_count][L].
 *   plx_apply_backward_rows     the two around the blur of plx_apply at vd = H, on the fp32 workspace of plx_apply_rows:
 *                               m x stride floats per plane, half of what the padded square gradient needs.
 * Rows are ALWAYS in the caller's order.  The two ranges are independent: disjoint, equal, nested or overlapping.  The
 * range tables are the slots of the rows calls, shared with them and across precisions; nothing new is stored per range.
 * The splat and the contraction report through plx_last_rows_kernels (rows_backward_splat_chunk_kernel /
 * rows_backward_splat_wide_kernel in the splat field, rows_backward_contract_chunk_kernel /
 * rows_backward_contract_wide_kernel in the slice field: the chunk shape up to 64 chunks, i.e. stride <= 256, the wide shape
 * above; a profiler shows the symbols with <float> or <float, D1> appended); the blur reports through plx_last_kernels.
 * PLX_ERR_STATE: a lattice that is not built, a sharded or merged build, a build that replayed "reference_growth", and under
 * stream capture a call that would have to build a range table or grow the workspace.  PLX_ERR_INVALID: a NULL pointer other
 * than d_filtered, nrhs < 1, a count < 1, a range outside [0, n), a pointer off 4-byte alignment, d_values off 16-byte
 * alignment, an output that aliases an input or the other output, and stride > 4096 (the wide contraction keeps four rows of
 * `stride` floats in the 64 KiB of LDS of a workgroup).  PLX_ERR_TOO_LARGE: m * stride, a_count * stride or b_count * stride
 * at or over 2^31.  Every argument is checked before any GPU work: a refused call writes nothing.  From the second call of a
 * (range pair, width) on, a call neither allocates nor synchronises (plx_device_bytes does not move) and is
 * graph-capturable.  No atomics, every output element written by exactly one thread: two calls with the same arguments are
 * bit-equal.
 * Two contracts.  (i) Bits, AS VALUES (-0.0 counted equal to +0.0): plx_backward_splat_rows equals plx_splat_rows of the
 * explicit half stack formed in float with one multiply per product element, in all `stride` columns; d_filtered equals
 * columns [0, L) of plx_apply_rows of that half stack, for every pair of ranges; the staged calls (splat, plx_blur at
 * vd = H, contract) give the bits of plx_apply_backward_rows.  (ii) Bar: every entry of d_grad_x is within
 * (k32 + 2 (L + 1)) 2^-23 of the size of the terms it sums (k32: the fp32 roundings along the deepest path of the product,
 * DESIGN.md section 22) of the contraction of a float64 filter of the half stack, and exactly 0 where no term reaches it.
 * The two one-sided results added into [n][d] agree with the padded square gradient to rounding; bit equality with it is not
 * promised.
 */
int plx_backward_splat_rows(plx_lattice *lat, const float *d_a, int64_t a_begin, int64_t a_count, const float *d_x,
                            int nrhs, float *d_values, void *stream);
int plx_backward_contract_rows(plx_lattice *lat, const float *d_values, const float *d_b, int64_t b_begin, int64_t b_count,
                               const float *d_x, int nrhs, float *d_grad_x, float *d_filtered /* may be NULL */, void *stream);
int plx_apply_backward_rows(plx_lattice *lat, const float *d_a, int64_t a_begin, int64_t a_count, const float *d_b,
                            int64_t b_begin, int64_t b_count, const float *d_x, int nrhs, float *d_grad_x,
                            float *d_filtered /* may be NULL */, void *stream);

/*
 * The reference's one-shot call (cpp:6-10 -> h:259-340): build a lattice for
 * d_ref, apply it to d_src, leave nothing behind.  `scratch` may be NULL or a
 * lattice object whose buffers are reused (avoids hipMalloc in steady state; it
 * is left built and usable).  The build knows it serves ONE MVM and leaves out
 * the stages that only pay back over several (vertex renumbering, axis-pair
 * tables of the blur): callers with more than a few MVMs per lattice use
 * plx_build + plx_apply.
 */
int plx_filter(plx_lattice *scratch, const float *d_src, const float *d_ref,
               int64_t n, int d, int vd, const float *h_taps, int ntaps,
               float *d_out, void *stream);

/*
 * Column-wise dot products of two row-major device matrices, d_out[c] = sum_r
 * a[r][c] * b[r][c]: the reduction a batched-CG caller needs per iteration
 * (GPyTorch's mBCG does it with torch ops).  Deterministic (fixed reduction
 * order).  d_work: plx_coldot_work_floats(vd) floats of device scratch.
 */
int plx_coldot(const float *d_a, const float *d_b, int64_t n, int vd, float *d_out, float *d_work, void *stream);
int64_t plx_coldot_work_floats(int vd);
/* Position gradient of one filter call, fused (replaces LatticeFilterGeneral.backward with a reference gradient,
 * bilateral_kernel.py:113-123): `lat` is built on d_ref [n][d] with the DERIVATIVE taps; d_g (the incoming gradient)
 * and d_src (the forward right-hand side) are [n][nrhs].  Writes d_grad_ref [n][d] and, unless NULL,
 * d_grad_src [n][nrhs].  The 2*nrhs*(1+d)-column stacked matrix and its filtered image are never stored: the splat
 * forms the stack from packed per-point records, slice and contraction are one kernel.  Column range 125..512
 * and 2*nrhs + d <= 62 (PLX_ERR_INVALID otherwise: use the three-call form below), single-shard lattices only. */
int plx_apply_backward(plx_lattice *lat, const float *d_g, const float *d_src, const float *d_ref, int nrhs,
                       float *d_grad_ref, float *d_grad_src, void *stream);
/* The two elementwise ends of the position gradient (bilateral_kernel.py:113-122), one pass each, row-major fp32:
 *   plx_backward_stack:    d_out[n][2L(1+d)] = [ g | g (x) x | src | src (x) x ]   (the matrix the filter is applied to)
 *   plx_backward_contract: d_grad_x[n][d] = -2 sum_l ( src x wg - src wgx + g x ws - g wsx ) from the filtered stack */
int plx_backward_stack(const float *d_g, const float *d_src, const float *d_x, int64_t n, int L, int d,
                       float *d_out, void *stream);
int plx_backward_contract(const float *d_g, const float *d_src, const float *d_x, const float *d_filtered,
                          int64_t n, int L, int d, float *d_grad_x, void *stream);
/* out = a * (K src) + b * src with (a, b) = d_scale_shift[0..1] read on the device: the (s K + sigma^2 I) v of a GP
 * solve in one call (the two scalars live in device memory so that no host synchronisation is needed to pass
 * hyper-parameters that are device tensors).  d_out must not alias d_src. */
int plx_apply_affine(plx_lattice *lat, const float *d_src, int vd, float *d_out, const float *d_scale_shift, void *stream);
/* plx_apply_affine that also returns d_dot[c] = <src[:, c], out[:, c]> (c < plx_values_stride(vd); padding entries are 0):
 * the p^T A p of a CG iteration comes out of the slice kernel's registers instead of a second pass over both
 * matrices.  2 <= vd <= 256.  d_work: plx_affine_dot_work_floats(lat, vd) floats of scratch. */
int64_t plx_affine_dot_work_floats(const plx_lattice *lat, int vd);
int plx_apply_affine_dot(plx_lattice *lat, const float *d_src, int vd, float *d_out, const float *d_scale_shift,
                         float *d_dot, float *d_work, void *stream);
/* d_dot may be NULL: the slice kernel's per-tile partial sums are then left in d_work -- plx_affine_dot_tiles(lat, vd) rows
 * of plx_values_stride(vd) floats -- for plx_cg_step_update_fused, which adds them up itself (one launch less). */
int plx_affine_dot_tiles(const plx_lattice *lat, int vd);
/* One batched-CG iteration's vector work with the coefficients formed on the device (all small arrays are float [vd],
 * `active` holds 1.0 / 0.0):
 *   plx_cg_step_update:    alpha = active ? rs / max(pAp, tiny) : 0;  X += alpha P;  R -= alpha AP;  rs_new = |R|^2
 *   plx_cg_step_direction: beta = active ? rs_new / max(rs, tiny) : 0;  P = R + beta P;
 *                          active_out = active and sqrt(rs_new) / b_norm > tol     (active_out != active) */
int plx_cg_step_update(float *d_x, float *d_r, const float *d_p, const float *d_ap, const float *d_rs, const float *d_pap,
                       const float *d_active, int64_t n, int vd, float *d_rs_new, float *d_alpha, float *d_work,
                       void *stream);
/* The same iteration without its two stand-alone reductions (round 6; vd = 4, 8, 12 or 16 -- rows of whole 16-byte chunks,
 * the widths solvers.khat_solve pads to; every pointer 16-byte aligned):
 *   plx_cg_step_update_fused     pAp comes as the PARTIAL sums plx_apply_affine_dot(d_dot = NULL) left behind (d_pap_partial:
 *                                ntiles = plx_affine_dot_tiles rows of vd floats); every workgroup adds them up itself, in
 *                                a fixed order.  |R|^2 leaves as partial sums in d_work (plx_cg_fused_work_floats(vd) floats).
 *   plx_cg_step_direction_fused  adds those up (every workgroup, fixed order), stores rs_new (d_rs_new != d_rs), beta and
 *                                active_out, and updates P.
 * Same arithmetic as the pair above except for the association of the column sums; deterministic.  Two launches fewer per
 * iteration: measured 11 % faster at n = 2e4, neutral at 1e5 ... 3e5, 0.3-0.5 % slower at n = 1e6 (every workgroup re-reads all
 * partial sums): a caller picks by size (simplex_gp_amd.solvers: up to 65,536 rows). */
int64_t plx_cg_fused_work_floats(int vd);
int plx_cg_step_update_fused(float *d_x, float *d_r, const float *d_p, const float *d_ap, const float *d_rs,
                             const float *d_pap_partial, int ntiles, const float *d_active, int64_t n, int vd,
                             float *d_alpha, float *d_work, void *stream);
int plx_cg_step_direction_fused(float *d_p, const float *d_r, const float *d_work, const float *d_rs, const float *d_active,
                                const float *d_b_norm, float tol, int64_t n, int vd, float *d_rs_new, float *d_beta,
                                float *d_active_out, void *stream);
/* ... and of the preconditioned iteration: <R, Z> as the partial sums plx_pcg_apply(d_rz = NULL) left in its d_work
 * (plx_pcg_rz_partial_rows(n, factor_type) rows of vd floats at float offset plx_pcg_rz_partial_offset(kp)), |R|^2 as
 * plx_cg_step_update_fused's partial sums; stores rz_new (!= d_rz), rr = |R|^2, beta, active_out; P = Z + beta P. */
int64_t plx_pcg_rz_partial_offset(int kp);
int plx_pcg_rz_partial_rows(int64_t n, int factor_type);
int plx_pcg_step_direction_fused(float *d_p, const float *d_z, const float *d_rz_partial, int nrz, const float *d_rr_partial,
                                 const float *d_rz, const float *d_active, const float *d_b_norm, float tol, int64_t n, int vd,
                                 float *d_rz_new, float *d_rr, float *d_beta, float *d_active_out, void *stream);
int plx_cg_step_direction(float *d_p, const float *d_r, const float *d_rs_new, const float *d_rs, const float *d_active,
                          const float *d_b_norm, float tol, int64_t n, int vd, float *d_beta, float *d_active_out,
                          void *stream);
/*
 * One Lanczos step with full re-orthogonalisation next to its MVM -- the variance cache of the reference's evaluation
 * (gpytorch.settings.fast_pred_var + max_root_decomposition_size(lanc_iter), experiments/train_simplexgp.py:63-72; GPyTorch
 * runs the recurrence with torch ops).  d_q: the basis, float [rows >= i + 2][ld] row-major, rows 0..i orthonormal; d_w:
 * A q_i on entry ([n], overwritten: on return the re-orthogonalised, un-normalised vector).  Writes d_alphas[i] =
 * q_i . A q_i, d_betas[i] = the norm of w after its components along rows i-1 and i (the alpha q_i and beta q_{i-1} terms
 * of the three-term recurrence) and then, in one classical Gram-Schmidt pass, along all rows 0..i have been removed, and
 * row i + 1 of d_q = w / max(beta_i, 1e-30).  Four launches, two streams of the basis, deterministic (fixed-order sums, no atomics).
 * i + 1 <= plx_lanczos_max_rows() (256); d_work: float [plx_lanczos_work_floats(n)] (< 0: n is larger than the 2,097,152
 * rows the step serves); ld >= n, a multiple of 4, d_q 16-byte aligned (columns n..ld-1 of the basis are never written).
 * Every argument is checked before any launch, by the checks of plx_lanczos_step_f64 below (one source for both,
 * csrc/plx_lanczos_kernels.h): PLX_ERR_INVALID also for a pointer off 4-byte alignment and for a d_w with any part
 * inside rows 0..i+1 of the basis, [d_q, d_q + (i + 2) ld) -- w is read and written while those rows are read and row
 * i + 1 is written.
 */
int plx_lanczos_max_rows(void);
int64_t plx_lanczos_work_floats(int64_t n);
int plx_lanczos_step(float *d_q, int64_t ld, float *d_w, int64_t n, int i, float *d_alphas, float *d_betas, float *d_work,
                     void *stream);
/*
 * The same step with every array in double (csrc/plx_lanczos_kernels.h with T = double): the recurrence and its order are
 * plx_lanczos_step's, the guard of the division is 1e-300 (row i + 1 of d_q = w / max(beta_i, 1e-300)).
 *   d_q       double [rows >= i + 2][ld], row-major, 16-byte aligned, ld >= n and ld % 2 == 0; columns n..ld-1 are never
 *             read for a result and never written
 *   d_w       double [n]: A q_i on entry, overwritten with the re-orthogonalised, un-normalised vector.  It must not
 *             overlap rows 0..i+1 of the basis, [d_q, d_q + (i + 2) ld)
 *   d_work    double [plx_lanczos_work_doubles(n)] (-1: n < 1 or more than the 2,097,152 rows the step serves)
 * Writes d_alphas[i], d_betas[i] and row i + 1 of d_q, and nothing else outside d_work.  Never allocates, never
 * synchronises (graph-capturable); deterministic: every sum is taken in a fixed order, no atomics.  i + 1 <=
 * plx_lanczos_max_rows() (256).  Every argument is checked before any launch; PLX_ERR_INVALID (plx_last_error names the
 * call): a NULL pointer, a pointer off 8-byte alignment or d_q off 16-byte alignment, an odd ld or ld < n, n < 1, i < 0 or
 * i + 1 > 256, an n the step does not serve, d_w overlapping the basis rows above.
 * plx_lanczos_shape_f64 (host only, no device): the rows per workgroup (span) and the workgroup count (groups =
 * ceil(n / span)) the step uses for n -- what plx_exact_splits is for the exact MVM: where the kernel shape changes,
 * without restating the rule.  PLX_ERR_INVALID where plx_lanczos_work_doubles refuses; span or groups may be NULL.
 */
int64_t plx_lanczos_work_doubles(int64_t n);
int plx_lanczos_shape_f64(int64_t n, int *span, int *groups);
int plx_lanczos_step_f64(double *d_q, int64_t ld, double *d_w, int64_t n, int i, double *d_alphas, double *d_betas,
                         double *d_work, void *stream);
/* The two vector updates of a batched CG iteration, one pass each (row-major [n][vd], per-column scalars on the
 * device):  plx_cg_update: X += P*alpha, R -= AP*alpha, d_rs_new[c] = sum_r R[r][c]^2 (d_work as for plx_coldot);
 *           plx_cg_direction: P = R + P*beta. */
int plx_cg_update(float *d_x, float *d_r, const float *d_p, const float *d_ap, const float *d_alpha,
                  int64_t n, int vd, float *d_rs_new, float *d_work, void *stream);
int plx_cg_direction(float *d_p, const float *d_r, const float *d_beta, int64_t n, int vd, void *stream);

/*
 * The exact kernel MVM, evaluated on the fly (nothing N x N is stored): the yardstick the lattice approximates.
 *   plx_exact_mvm:  out[i][c] = sum_j k(|x1_i - x2_j|^2) v[j][c]
 *   plx_exact_grad: grad_x1[i][:] = sum_j 2 k'(|x1_i - x2_j|^2) (x1_i - x2_j) (g_i . v_j)
 * x1 [n1][d], x2 [n2][d], v [n2][t], g and out [n1][t], grad_x1 [n1][d]: fp32, row-major, contiguous, device memory;
 * positions already divided by the lengthscale.  1 <= n1, n2 < 2^31, 1 <= d <= PLX_MAX_DIM, t >= 1.  k is a profile of
 * the squared distance d2 (the project's own, stencil.py): RBF exp(-d2) (not GPyTorch's exp(-d2 / 2)); Matern-nu with
 * r = sqrt(d2): e^-r, (1 + sqrt3 r) e^-sqrt3 r, (1 + sqrt5 r + 5/3 r^2) e^-sqrt5 r.  A Matern-1/2 pair at r = 0 adds 0
 * to the gradient.  grad_x2 is plx_exact_grad with the roles swapped (x1 <-> x2, g <-> v).
 * Stateless: d_work is the caller's, at least plx_exact_work_bytes(n1, n2, d, t) bytes (monotone in every size, at most
 * 16 MB; < 0 for sizes outside the limits), so nothing is allocated and the calls are graph-capturable.  Deterministic:
 * no float atomics (a split j range is summed slice by slice in a fixed order).  Every argument is checked before any
 * GPU work (PLX_ERR_INVALID, PLX_ERR_DIM for d).
 * plx_exact_splits: the number of slices the j range of that call is cut into (1: written directly, no workspace
 * used; > 1: slabs [splits][n1][t or d] in d_work, summed in slice order); -1 where plx_exact_work_bytes refuses.  A
 * host function, no device needed: a test knows which path a call takes without restating the rule.
 */
enum { PLX_PROFILE_RBF = 0, PLX_PROFILE_MATERN12 = 1, PLX_PROFILE_MATERN32 = 2, PLX_PROFILE_MATERN52 = 3 };
int64_t plx_exact_work_bytes(int64_t n1, int64_t n2, int d, int t);
int plx_exact_splits(int64_t n1, int64_t n2, int d, int t);
int plx_exact_mvm(const float *d_x1, int64_t n1, const float *d_x2, int64_t n2, int d, int profile,
                  const float *d_v, int t, float *d_out, void *d_work, int64_t work_bytes, void *stream);
int plx_exact_grad(const float *d_x1, int64_t n1, const float *d_x2, int64_t n2, int d, int profile,
                   const float *d_g, const float *d_v, int t, float *d_grad_x1, void *d_work, int64_t work_bytes,
                   void *stream);
/*
 * The same two products with every array in double (csrc/plx_exact_f64.hip): the formulas, profiles and conventions
 * above (a Matern-1/2 pair at r = 0 adds 0 to the gradient; grad_x2 is plx_exact_grad_f64 with the roles swapped).
 * x1, x2, v, g, out and grad_x1 are double, row-major, contiguous, device memory, 8-byte aligned; every operation is a
 * double operation (exp and sqrt in double, direct differences, each tile of 64 rows of x2 summed apart from the running
 * sum): nothing is rounded through fp32.  The limits, the argument checks, their order and their return codes are those
 * of plx_exact_mvm / plx_exact_grad, all made before any GPU work.
 * Stateless: d_work is the caller's, at least plx_exact_work_bytes_f64(n1, n2, d, t) bytes (a multiple of 8, monotone in
 * every size, at most 16 MiB; -1 exactly where plx_exact_work_bytes refuses), so nothing is allocated and the calls are
 * graph-capturable.  Deterministic: no float atomics, every output element is written by one thread, two identical calls
 * are bit-equal.
 * plx_exact_splits_f64: the number of slices the j range of that call is cut into (1: written directly, no workspace
 * used; > 1: slabs [splits][n1][t or d] of doubles in d_work, summed in slice order by a second kernel); -1 where
 * plx_exact_work_bytes_f64 refuses.  A host function, and the one the launch itself calls.  The slabs are doubles under
 * the same 16 MiB, so a call may be cut into fewer slices than the fp32 call of the same sizes.
 */
int64_t plx_exact_work_bytes_f64(int64_t n1, int64_t n2, int d, int t);
int plx_exact_splits_f64(int64_t n1, int64_t n2, int d, int t);
int plx_exact_mvm_f64(const double *d_x1, int64_t n1, const double *d_x2, int64_t n2, int d, int profile,
                      const double *d_v, int t, double *d_out, void *d_work, int64_t work_bytes, void *stream);
int plx_exact_grad_f64(const double *d_x1, int64_t n1, const double *d_x2, int64_t n2, int d, int profile,
                       const double *d_g, const double *d_v, int t, double *d_grad_x1, void *d_work,
                       int64_t work_bytes, void *stream);

/*
 * Preconditioned batched CG: the reference trains with gpytorch.settings.max_preconditioner_size(100)
 * (experiments/train_simplexgp.py:36, configs/simplexgp.yml), i.e. every solve of (s K + sigma^2 I) is preconditioned by
 * P = L L^T + sigma^2 I, L [n][k] the rank-k pivoted Cholesky factor of s K (GPyTorch builds and applies it with torch
 * ops).  These entry points are that work as native passes.  The factor is handed over TRANSPOSED:
 *   d_lt   float [kp][ld] row-major = L^T; kp = k rounded up to a multiple of 16 (the extra rows zero), ld = n rounded up
 *          to a multiple of 64 (the tail of every row zero), 16-byte aligned; the n dimension in the same row order as
 *          the CG vectors (solvers.py keeps everything in lattice row order, so nothing is permuted per iteration);
 *   t      columns of the CG vectors, 1..16, row-major [n][t];
 *   d_work plx_pcg_work_floats(n, kp, t) floats of scratch.
 * One application Z = P^-1 R = (R - L C^-1 L^T R) / sigma^2, C = sigma^2 I + L^T L, is two streaming passes over L^T:
 *   plx_pcg_project   T [kp][16] = C^-1 (L^T R): the products on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32
 *                     products, fp32 accumulation), per-workgroup partial sums added in fp64 in a fixed order, then the
 *                     kp x kp solve with d_cinv = C^-1 in fp64 [kp][kp] (symmetric; identity / sigma^2 on the padding);
 *   plx_pcg_apply     Z = (d_scale[0] R - L T) d_scale[1] (k = columns of L actually used) and, unless NULL,
 *                     d_rz[c] = <R[:, c], Z[:, c]> from the same registers.  d_scale: two floats in device memory.
 *   plx_pcg_step_direction   beta = active ? rz_new / rz : 0; P = Z + beta P; active_out = active and
 *                     sqrt(rr) / b_norm > tol (rr = |R|^2 as plx_cg_step_update returns it: the TRUE residual).
 * plx_cg_step_update is used unchanged with rs := rz.  Deterministic (no atomics).
 * factor_type: the factor's storage, PLX_FACTOR_F32 or PLX_FACTOR_F16 (IEEE half, same [kp][ld] layout; made from the fp32
 * factor by plx_pcg_factor_to_half).  Both passes are bound by streaming the factor, so the half-width copy halves them.
 * A preconditioner only has to be symmetric positive definite and the same matrix wherever it is used: a caller that
 * stores L in fp16 must form C = sigma^2 I + L^T L, the log-determinant and its probe vectors from that SAME rounded L
 * (solvers.LatticePreconditioner does); products and accumulation are fp32 either way.
 */
enum { PLX_FACTOR_F32 = 0, PLX_FACTOR_F16 = 1 };
int64_t plx_pcg_work_floats(int64_t n, int kp, int t);
int plx_pcg_project(const void *d_lt, int factor_type, int64_t ld, int kp, const float *d_r, int64_t n, int t,
                    const double *d_cinv, float *d_t, float *d_work, void *stream);
int plx_pcg_apply(const void *d_lt, int factor_type, int64_t ld, int kp, int k, const float *d_r, int64_t n, int t,
                  const float *d_t, const float *d_scale, float *d_z, float *d_rz, float *d_work, void *stream);
int plx_pcg_factor_to_half(const float *d_lt, int64_t ld, int kp, void *d_lt_half, void *stream);
int plx_pcg_step_direction(float *d_p, const float *d_z, const float *d_rz_new, const float *d_rz, const float *d_rr,
                           const float *d_active, const float *d_b_norm, float tol, int64_t n, int vd, float *d_beta,
                           float *d_active_out, void *stream);
/*
 * The same application in float64, next to the float64 CG solve (callers detect it by symbol; the version string is
 * unchanged).  The factor is the one plx_pchol_* builds and STAYS fp32 (d_lt float [kp][ld] exactly as above: kp a multiple
 * of 16 up to 1024, ld >= n a multiple of 64, zero tails, 16-byte aligned): an fp32 entry converts to double exactly, so
 * P = L L^T + sigma^2 I is one matrix whatever precision applies it.  Everything else is double: vectors double [n][t]
 * row-major (1 <= t <= 16, 8-byte aligned) in the SAME row order as the factor's n dimension, whatever that order is
 * (solvers.LatticePreconditioner64 keeps both in the caller's order, like every fp64 call); G and T double [kp][16], of
 * which a call writes columns 0..t-1; d_cinv double [kp][kp]; d_work plx_pcg_work_doubles(n, kp, t) doubles (-1 outside
 * the limits above, monotone inside).
 *   plx_pcg_gram_f64      G = L^T R: fp64 products of the converted entries with fp64 accumulation on the matrix cores
 *                         (v_mfma_f64_16x16x4_f64), per-workgroup partial sums added in a fixed order.  With the factor's
 *                         own columns as R (tiles of 16) it forms L^T L, hence C = sigma^2 I + L^T L, in double;
 *   plx_pcg_project_f64   T = C^-1 (L^T R): the gram pass, then the kp x kp product with d_cinv in double;
 *   plx_pcg_apply_f64     Z = (d_scale[0] R - L T) d_scale[1] (k <= kp = columns of L actually used: rows k.. of T are not
 *                         read; d_scale two doubles in device memory) and, unless d_rz is NULL, d_rz[c] = <R[:, c], Z[:, c]>
 *                         from the same registers, complete on return (one partial row per workgroup, fixed-order final
 *                         sum).  d_z != d_r.  Rows of R and Z move as 16-byte pairs when t is even and both are 16-byte
 *                         aligned;
 *   plx_pcg_step_direction_f64   beta = active ? rz_new / max(rz, 1e-300) : 0; P = Z + beta P; active_out = active and
 *                         sqrt(rr) / b_norm > tol: plx_cg_step_direction_f64 with Z as the source and the TRUE residual
 *                         |R|^2 in the test (1 <= vd <= 256, every array double, active_out != active).
 * plx_cg_step_update_f64 is used unchanged with rs := rz.  No allocation, no synchronisation (graph-capturable), no float
 * atomics: two calls with the same arguments are bit-equal.  Every argument is checked before any launch: a NULL pointer,
 * t or vd out of range, n < 1, k outside 0..kp, a factor off the shape contract, a pointer off its alignment and the
 * aliasings named above are PLX_ERR_INVALID.
 * Error bars (U = 2^-52; tests/test_pcg_f64_gpu.py): a gram entry (n + 4) U sum_i |L_ij R_ic|; a project entry
 * (n + kp + 8) U sum_q |Cinv_jq| sum_i |L_iq R_ic|; an apply entry (k + 6) U |s1| (|s0 r| + sum_j |L_ij T_jc|); rz
 * (n + 4) U sum_r |R Z|.
 */
int64_t plx_pcg_work_doubles(int64_t n, int kp, int t);
int plx_pcg_gram_f64(const float *d_lt, int64_t ld, int kp, const double *d_r, int64_t n, int t, double *d_g, double *d_work,
                     void *stream);
int plx_pcg_project_f64(const float *d_lt, int64_t ld, int kp, const double *d_r, int64_t n, int t, const double *d_cinv,
                        double *d_t, double *d_work, void *stream);
int plx_pcg_apply_f64(const float *d_lt, int64_t ld, int kp, int k, const double *d_r, int64_t n, int t, const double *d_t,
                      const double *d_scale, double *d_z, double *d_rz, double *d_work, void *stream);
int plx_pcg_step_direction_f64(double *d_p, const double *d_z, const double *d_rz_new, const double *d_rz, const double *d_rr,
                               const double *d_active, const double *d_b_norm, double tol, int64_t n, int vd, double *d_beta,
                               double *d_active_out, void *stream);
/*
 * The factor itself, built in batches of speculated pivots.  The sequential algorithm (GPyTorch's pivoted_cholesky, one
 * kernel row = one single-column MVM per pivot) is reproduced exactly, but nb <= 16 pivots share ONE nb-column MVM:
 *   plx_pchol_select        d_cand[0..nb) = the nb largest entries of the residual diagonal d_diag [n], ties by LOWER
 *                           d_rank[i] (NULL: by lower i) -- pass the lattice's point permutation so that ties fall as
 *                           torch.argmax breaks them on the caller-order vector; the largest entry that is NOT a
 *                           candidate is kept in d_work (it bounds every non-candidate for the whole batch: steps only
 *                           lower entries).  May run as soon as the previous batch's plx_pchol_factor_batch is enqueued;
 *   plx_pchol_onehot        d_rhs [n][t] = the nb one-hot columns (t >= nb; the caller runs the MVM on it);
 *   plx_pchol_factor_batch  d_rows [n][t] = K d_rhs.  Panel update against the m_done finished columns
 *                           (d_scale[0] d_rows - L L[cand]^T, one pass over them), then the in-batch steps in pivot
 *                           order: column m_done + b = panel row of the step's pivot / sqrt(pivot) (zero if the pivot is
 *                           <= tol_abs), residual diagonal updated.  Which candidate a step takes is the argmax of the
 *                           updated diagonal (the sequential algorithm may take the candidates in another order than
 *                           their values at the start of the batch suggest).  The steps whose argmax is CERTAIN from the
 *                           candidates' own entries -- the largest unused candidate still lies above the largest entry
 *                           outside the batch, which a step can only lower -- are planned on the nb x nb block of the
 *                           panel and written in ONE pass over the n-vectors ("planned" steps, >= 1).  exact_steps != 0:
 *                           the remaining candidates are then tried one launch per step, the argmax looked up on the
 *                           device among them; the batch ends when the argmax is an entry whose kernel row is not in
 *                           it.  exact_steps == 0: the batch ends with the plan.  d_accepted (device int32 [2]) =
 *                           {columns written, planned steps}; the caller reads it back once per batch, carries on from
 *                           m_done + accepted and passes exact_steps = 0 while whole batches come out planned (sparse
 *                           kernel rows: a column touches few other candidates).
 * d_work: plx_pchol_work_bytes(ld, kp) bytes, the same buffer for the three calls of a batch.
 */
int64_t plx_pchol_work_bytes(int64_t ld, int kp);
int plx_pchol_select(const float *d_diag, const uint32_t *d_rank, int64_t n, int nb, int64_t ld, int kp, int32_t *d_cand,
                     void *d_work, void *stream);
int plx_pchol_onehot(const int32_t *d_cand, int nb, int64_t n, int t, float *d_rhs, void *stream);
int plx_pchol_factor_batch(float *d_lt, int64_t ld, int kp, int m_done, const float *d_rows, int t, const float *d_scale,
                           const int32_t *d_cand, int nb, float *d_diag, const uint32_t *d_rank, int64_t n, float tol_abs,
                           int exact_steps, int32_t *d_accepted, void *d_work, void *stream);

/* Copy one structure array to host memory (parity tests, debugging).
 * h_dst must hold `bytes` bytes, which must equal the array's size. */
int plx_export(plx_lattice *lat, int which, void *h_dst, int64_t bytes, void *stream);
/* PLX_ARRAY_POINT_PERM device to device (uint32 [n]): lets a caller permute its vectors into lattice row
 * order on the GPU without a host round trip. */
int plx_copy_point_perm(plx_lattice *lat, void *d_dst, void *stream);
/* size in bytes of an exportable array, or -1 */
int64_t plx_export_bytes(const plx_lattice *lat, int which);

/* Select a kernel variant by name: for A/B measurements in one process -- the defaults are the shipped configuration.
 * plx_tune sets the PROCESS DEFAULT of a switch.  A lattice never reads the defaults while it works: every build
 * (plx_build, plx_build_local, plx_filter) starts by copying them into the lattice, and every later call on that lattice
 * (its merge, tables, MVMs, exports) runs under that copy -- so a plx_tune call changes nothing for lattices that are
 * already built, two lattices built under different settings keep their own, and a thread that tunes while another
 * thread is inside a plx_* call on a built lattice does not disturb it (concurrent plx_tune and build calls still need
 * the caller's own ordering: the copy is a plain struct copy).  plx_lattice_tune changes a switch in ONE lattice's copy,
 * effective from its next call until its next build (A/B of MVM-side variants over the same tables).  Keys (default):
 *   "sort_points" (1; 0 keeps the caller's point order), "vertex_order" (1: vertices numbered along the Morton curve of their blur-axis coordinates where
 *   that pays, 65536 <= m <= 0.9 n (d+1); 0: always by first touch; 2: always Morton -- vertex ids are internal, the
 *   PLX_ARRAY_* exports are in whichever numbering the build used), "insert_dedupe" (2 = every key of a wave probes the table once: lanes with equal keys are grouped by hash ballots; 1 = runs of
 *   equal NEIGHBOURING lanes probe once; 0 = every lane probes), "compact_nbr" (1 = when under a quarter of the neighbour slots exist;
 *   0 never, 2 always), "blur_vpt" (4; vertices per thread at vd = 1: 2 or 4, anything else selects the general kernel),
 *   "blur_small" (1), "blur_narrow" (1), "blur_multi" (1 = the wide-row blur kernels from 17 chunks per row; 2 = from 32, the
 *   gate of rounds 1-5), "blur_fuse" (1), "blur_fuse_vec" (1 = two blur axes per launch
 *   for rows of 2..4 chunks; 0 = one), "splat_direct" (1), "splat_group" (1), "splat_wide" (1 = the row-parallel splat from 17 chunks per
 *   row; 2 = from 32),
 *   "block_path" (1 = block tables for vd = 1 when corners share vertices; 0 never, 2 whenever representable),
 *   "block_e" (0 = corners per thread of the block kernels chosen per lattice; 16 or 24: a block holds 256 * e corners),
 *   "block_dense_combine" (1), "unpermute_gather" (1), "nbr_bitmap" (1 = neighbour lookups test a
 *   slot-occupancy bitmap before the hash table when m >= 2^22; 0 never, 2 always), "splat_first" (1 = single-column splat by
 *   first-touch stores + a short extras list when m >= 0.9 nnz; 0 never, 2 whenever representable, 3 = 2 with scattered
 *   stores), "perm_rows" (1 = multi-column row permutations by 16-byte chunks / LDS-transposed whole-line stores; 0 = the
 *   per-float forms), "reference_growth" (0; 1 = replay the reference CPU path's table-growth quirk: plx_reference_growth_info; 2 = the same by
 *   running every lookup, the checker of 1), "blur_active" (1: wide rows on sparse lattices -- centre tap 1 -- blur only the vertices with a neighbour on the axis, in place; 0 never, 2 whenever representable),
 *   "contract_v" (1 = the fused backward's slice + contraction with the corner count
 *   compiled in; 0 = the run-time form),
 *   and the round-5 build switches "nbr_sliced" (1), "nbr_seed" (1), "assign_evid" (1): DESIGN.md 2.  (Round 6 removed
 *   "hash_v", "table_fp", "flag_own" and "insert_v" with the measured-loser code paths behind them: the linear hash,
 *   fingerprints, own-mark flags and the point-per-thread insert are what every build uses.  Twelve more settled A/B
 *   levers went the same way later, each fixed at what had been its default: "xcd_remap" (tiles remapped so that every XCD
 *   owns a contiguous eighth; the multi-item wide-row blur keeps plain order), "readback_spin" (counts come back through
 *   the mailbox), "order_compact" (point-order keys over exactly the bits each coordinate's range needs), "order_zcurve"
 *   (points along the Z-curve of their rounded lattice coordinates), "order_sample" (that range from every 8th point, from
 *   65,536 points up), "embed_vrange" (the vertex-coordinate range comes from a pass of its own), "insert_xcd" (the hashed
 *   insert in plain tile order, the id lookup remapped), "insert_plane_fast" (the d+1 axis planes of a run of vertices are
 *   adjacent workgroups of the neighbour lookups wherever the grid allows), "nbr_symmetric" (positive taps looked up, hits
 *   mirrored), "nbr_window" (on Morton-numbered lattices a neighbour lookup first binary-searches 512 sorted vertex codes
 *   on the target's side of the vertex), "scatter_store" (plain stores out of the block slice) and "blk_sort" (block
 *   tables sorted as packed keys, 5 bits per pass, 512 threads; (key, value) pairs where the packed key does not fit).)
 * The diagnostic ablations "splat_ablate" / "blur_ablate" / "block_ablate" exist only in libplx_diag.so (make diag).
 * Unknown keys return PLX_ERR_INVALID. */
int plx_tune(const char *key, int value);
int plx_lattice_tune(plx_lattice *lat, const char *key, int value);

/* Names of the kernels the last plx_splat / plx_blur / plx_slice (or plx_apply) on this lattice launched, as
 * "splat=a+b;blur_axis=c;slice=d;vertex_order=morton|first_touch" -- the names rocprofv3 --kernel-trace shows (without
 * template arguments) and the vertex numbering of the last build, so that a bench line can name what actually ran. */
int plx_last_kernels(const plx_lattice *lat, char *buf, int cap);
/* The splat / slice tables of a built lattice (block tables, their vertex-sorted half, the vertex-sorted CSR) are built
 * by their first user: the first plx_splat / plx_slice / plx_apply that needs them, on that call's stream -- a CG-only
 * caller never pays for single-column tables and vice versa.  plx_prepare builds, on `stream`, everything an MVM with
 * vd columns will read, so that the first MVM costs what every later one does (and so that a profile can time the
 * tables apart from the MVM).  Idempotent. */
int plx_prepare(plx_lattice *lat, int vd, void *stream);
/* Block rows of the lattice's block tables (coarse lattices: the owned points are cut into blocks, a block row = one
 * distinct vertex of one block), or 0 when the tables have not been built (see plx_prepare) or the lattice uses the
 * vertex-sorted CSR path instead.  A pure query: no launch, no synchronisation. */
int64_t plx_block_rows(const plx_lattice *lat);

/* Self test of the build's stable radix sort (plx_radix.h) on the current device: n (key, position) pairs with many
 * duplicate keys of key_bytes (4 or 8) bytes and end_bit significant bits are sorted and checked on the device --
 * ascending, equal keys in input order, every value still with its key.  *mismatches = offending positions (0 = pass).
 * Synchronises the stream.  For tests; no lattice needed. */
int plx_selftest_sort(int64_t n, int key_bytes, int end_bit, uint64_t seed, void *stream, int64_t *mismatches);

/* Per-stage device time of the last plx_build on this lattice, in ms, in the
 * order {order+embed, insert, number, ids, neighbours, csr}; 0 when timing is off.
 * plx_set_timing(lat, 1) turns hipEvent timing on (adds event records only). */
int plx_set_timing(plx_lattice *lat, int on);
int plx_build_times(const plx_lattice *lat, float *h_ms6);
/* Per-stage device time of the last plx_apply (timing on), in ms: {splat (scan +
 * fix-up launch), blur (all d+1 launches), slice}.  One hipEvent pair per stage
 * on the apply stream, so a stage time divided by its launch count is directly
 * comparable with rocprofv3's per-kernel average.  Synchronises on the last event. */
int plx_apply_times(plx_lattice *lat, float *h_ms, int cap, int *count);

#ifdef __cplusplus
}
#endif
#endif /* PLX_H */
