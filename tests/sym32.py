"""TEST HELPER: the fp32 bars of the transposed and the symmetrised lattice products, and a numpy float32 model of them.

Bars (per entry, against tests/sym64.Sym64 in float64):
    K^T v   within ENTRY * T_t                 T_t = Sym64.kt.terms64(v)
    K_s v   within (ENTRY + 2^-24) * T_s       T_s = Sym64.terms64(v)
    an entry is exactly 0 where its T is 0.
ENTRY is the per-entry bar of the forward fp32 product (tests/test_forward_fp64.py, restated here because that module needs
a GPU to import its fixtures): the transposed chain is the forward chain of another tap order, so it gets the same bar.  The
symmetrised plane is 0.5 (F + R): the two chains' bars averaged -- ENTRY (T_k + T_t) / 2 = ENTRY T_s -- plus one rounding of
the sum, at most 2^-24 |F + R| / 2 <= 2^-24 T_s after the (linear, non-negative) slice.  REL is the forward product's rel-L2
bar.

model32: both products formed in numpy float32 from the S, blur and tap data of a Sym64, every intermediate rounded to
float32 (each product w * x rounded, each partial sum rounded: no fused multiply-add, the looser of the two forms a GPU
kernel may take).  Checker only.
"""
import numpy as np

from tests.lattice64 import entry_ratio

ENTRY = 1.8e-6            # tests/test_forward_fp64.py ENTRY
REL = 1.6e-6              # tests/test_forward_fp64.py REL
U32 = 2.0 ** -24
ENTRY_SYM = ENTRY + U32


def spmm32(A, X):
    """A @ X for a scipy CSR matrix A and a float32 array X, carried in float32: row by row, entry by entry in the order the
    CSR stores them, acc = fl(acc + fl(a * x)).  Vectorised over the rows: step k handles the k-th stored entry of every
    row that has one."""
    A = A.tocsr()
    X = np.asarray(X, np.float32)
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    data = A.data.astype(np.float32)           # (weights and taps are fp32 values: exact)
    lens = np.diff(indptr)
    acc = np.zeros((A.shape[0],) + X.shape[1:], np.float32)
    for k in range(int(lens.max()) if lens.size else 0):
        rows = np.nonzero(lens > k)[0]
        e = indptr[rows] + k
        term = (data[e][:, None] * X[indices[e]]).astype(np.float32)
        acc[rows] = (acc[rows] + term).astype(np.float32)
    return acc


def model32(op, v):
    """(K^T v, K_s v) in float32 for a tests/sym64.Sym64 `op`: splat once, the forward chain F through op.k.blurs and the
    reverse chain R through op.kt.blurs (the axes d .. 0 with mirrored taps), the plane 0.5 (F + R) with the sum rounded
    once, each sliced and divided by 1 + 2^-d in float32."""
    v32 = np.asarray(v, np.float32)
    St = op.k.S.T.tocsr()
    splat = spmm32(St, v32)
    F, R = splat, splat
    for B in op.k.blurs:
        F = spmm32(B, F)
    for B in op.kt.blurs:
        R = spmm32(B, R)
    mean = (np.float32(0.5) * (F + R).astype(np.float32)).astype(np.float32)
    denom = np.float32(op.k.denom)
    kt = (spmm32(op.k.S, R) / denom).astype(np.float32)
    ks = (spmm32(op.k.S, mean) / denom).astype(np.float32)
    return kt, ks


def ratios(op, v, got_t, got_s):
    """(entry ratio of K^T, entry ratio of K_s, T_t, T_s) against the float64 operators of `op` on the float32 input `v`."""
    v64 = np.asarray(v, np.float32).astype(np.float64)
    Tt, Ts = op.kt.terms64(v64), op.terms64(v64)
    et = entry_ratio(got_t, op.kt.apply_staged(v64), Tt) if got_t is not None else None
    es = entry_ratio(got_s, op.apply_staged(v64), Ts) if got_s is not None else None
    return et, es, Tt, Ts
