// plx_diag_kernels.h -- the true diagonal of the lattice operator, K_ii, per point, from the tables of a plain build
// (plx_diag / plx_diag_f64, include/plx.h; the entry points and their argument checks are in plx_api.hip).  One templated
// body, instantiated for float by plx_diag.hip and for double by plx_diag_f64.hip.
//
//   K = S B_d ... B_0 S^T / (1 + 2^-d), so with the corners v_0..v_d and the weights w_0..w_d of point i
//   K_ii = (1 / (1 + 2^-d)) sum_{a,b} w_a w_b (B_d ... B_0)[v_a, v_b].
//
// An entry of the blur product is a sum over paths of one hop per axis, axis d first and axis 0 last.  A hop of shift t in
// [-r, r] goes through the neighbour table (slot t + r below zero, t + r - 1 above: -r..-1, 1..r) and costs the tap
// c[t + r]; a path that meets an absent neighbour contributes nothing.  The d + 1 blur directions sum to zero and satisfy no
// other relation, so the shift vectors that lead from corner a to corner b of one simplex are t_j = c + s_j: s a fixed
// pattern of the pair, c every integer that keeps all t_j in [-r, r] -- at most 2 r + 1 paths per ordered pair.
//
// The pattern.  Corner k - 1 is the +1 neighbour of corner k along exactly one axis, j_k (the coordinate of rank d + 1 - k
// in the point's rank permutation).  The kernel does not decode the point records: it FINDS j_k by looking corner k - 1 up
// among the d + 1 "+1" neighbours of corner k in the table the walks go through anyway, and keeps pos[j_k] = k (the one
// axis that is no j_k keeps pos 0).  Then v_b = v_a - sum_{a < k <= b} dir(j_k) for a < b:
//   a < b   s_j = -1 where a < pos[j] <= b, else 0;   c in [-r + 1, r]
//   a > b   s_j = +1 where b < pos[j] <= a, else 0;   c in [-r, r - 1]
//   a = b   s = 0;                                    c in [-r, r]
// Order 0 (r = 0) leaves the pairs a = b at c = 0 and reads no table: c_0^(d+1) sum_a w_a^2 / (1 + 2^-d).
//
// Work.  A walk is a chain of d + 1 dependent 4-byte gathers: latency, not bytes.  A group of G = 2^glog lanes (4..64, the
// (pair, c) item count rounded up to a power of two) serves one point; its lanes stride over the (d+1)^2 (2r+1) items, so a
// wave keeps 64 independent chains in flight.  Per point the corners, the weights (converted exactly to T) and pos[] are
// staged once in LDS, the taps once per workgroup (LDS, not the kernel argument: they are indexed per lane).  Every lane
// sums its items in item order, then the group adds its lanes up by a butterfly of fixed shape; lane 0 divides by
// 1 + 2^-d and stores.  No atomics, every output element written by one thread, sums in a fixed order: bitwise
// reproducible.  Points are taken in lattice order; a point outside the caller's row range does nothing after one load of
// perm.  No workspace, no allocation, no host read-back: legal under stream capture.
#pragma once

#include "plx_kernels.h"

#include <math.h>

namespace plx {

template <typename T>
__global__ __launch_bounds__(kBlock) void diag_kernel(const int *__restrict__ evid, const float *__restrict__ ew,
                                                      const int *__restrict__ nbr, const uint32_t *__restrict__ perm, int n,
                                                      int d1, int r, int64_t mstride, int glog, int64_t row_begin,
                                                      int64_t row_count, TapArgs taps, T denom, T *__restrict__ out,
                                                      int ntiles)
{
    extern __shared__ __align__(16) unsigned char diag_smem[];
    const int tile = tile_index(ntiles);
    if (tile < 0) return;                                     // (the whole workgroup: no barrier is left waiting)
    const int ppb = kBlock >> glog, G = 1 << glog, R = 2 * r + 1;
    const int grp = (int)threadIdx.x >> glog, lane = (int)threadIdx.x & (G - 1);
    T *s_taps = reinterpret_cast<T *>(diag_smem);                                   // [2 PLX_MAX_ORDER + 1 rounded up to 18]
    T *s_w = s_taps + 2 * PLX_MAX_ORDER + 2 + grp * d1;                              // [ppb][d1], this group's row
    int *s_vid = reinterpret_cast<int *>(s_taps + 2 * PLX_MAX_ORDER + 2 + ppb * d1) + grp * d1;   // [ppb][d1]
    int *s_pos = s_vid + ppb * d1;                                                   // [ppb][d1]

    const int64_t p = (int64_t)tile * ppb + grp;
    bool live = p < n;
    int64_t orow = p;
    if (live && perm) {                                       // caller rows: only the points of the range work
        orow = (int64_t)perm[p] - row_begin;
        live = orow >= 0 && orow < row_count;
    }
    if ((int)threadIdx.x < R) s_taps[threadIdx.x] = (T)taps.c[threadIdx.x];
    if (live)
        for (int k = lane; k < d1; k += G) {
            s_vid[k] = evid[(size_t)k * n + p];
            s_w[k] = (T)ew[(size_t)k * n + p];
            s_pos[k] = 0;
        }
    __syncthreads();
    if (live && r > 0)
        for (int q = lane; q < (d1 - 1) * d1; q += G) {       // (corner k >= 1, axis j): is corner k - 1 the +1 neighbour?
            const int k = 1 + q / d1, j = q - (k - 1) * d1;
            if (nbr[((int64_t)j * 2 * r + r) * mstride + s_vid[k]] == s_vid[k - 1]) s_pos[j] = k;
        }
    __syncthreads();

    T acc = (T)0;
    if (live) {
        const int items = d1 * d1 * R;
        for (int item = lane; item < items; item += G) {
            const int a = item / (d1 * R), rem = item - a * (d1 * R);
            const int b = rem / R, c = rem - b * R - r;
            if ((a < b && c == -r) || (a > b && c == r)) continue;      // no such path: a shift would leave [-r, r]
            const int lo = a < b ? a : b, hi = a < b ? b : a, sgn = a < b ? -1 : 1;
            int x = s_vid[a];
            T prod = (T)1;
            for (int j = d1 - 1; j >= 0 && x >= 0; --j) {
                const int pj = s_pos[j];
                const int t = c + ((pj > lo && pj <= hi) ? sgn : 0);
                if (t != 0) x = nbr[((int64_t)j * 2 * r + (t < 0 ? t + r : t + r - 1)) * mstride + x];
                prod *= s_taps[t + r];
            }
            if (x >= 0) acc += (s_w[a] * s_w[b]) * prod;
        }
    }
    // the lanes of a group, added up in a fixed shape (a group never straddles a wave; idle groups carry zeros)
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (live && lane == 0) out[orow] = acc / denom;
}

// LDS of a launch: the taps (18 T), then per point of the workgroup d + 1 weights, ids and positions
template <typename T> static size_t diag_lds_bytes(int d1, int glog)
{
    return (size_t)(2 * PLX_MAX_ORDER + 2) * sizeof(T) + (size_t)(kBlock >> glog) * d1 * (sizeof(T) + 8);
}

// Arguments checked by the entry points.  lattice_rows: out[p] for the lattice position p, the whole [0, n).
template <typename T>
int diag_impl(plx_lattice *L, int64_t row_begin, int64_t row_count, bool lattice_rows, T *d_out, hipStream_t stream)
{
    const int d1 = L->d + 1, r = L->order;
    const int64_t items = (int64_t)d1 * d1 * (2 * r + 1);
    int glog = 2;
    while (glog < 6 && (1 << glog) < items) ++glog;
    const int ppb = kBlock >> glog;
    const int ntiles = ceil_div(L->n, ppb);
    const T denom = (T)1 + (T)ldexp(1.0, -L->d);
    diag_kernel<T><<<tile_grid(ntiles), kBlock, diag_lds_bytes<T>(d1, glog), stream>>>(
        L->evid.as<int>(), L->ew.as<float>(), L->nbr.as<int>(), lattice_rows ? nullptr : L->perm.as<uint32_t>(), (int)L->n, d1, r,
        L->mstride, glog, row_begin, row_count, L->taps, denom, d_out, ntiles);
    PLX_HIP_TRY(hipGetLastError());
    return PLX_OK;
}

}  // namespace plx
