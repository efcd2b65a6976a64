"""TEST HELPER: the one-sided float64 position gradient of the rectangular product (plx_apply_backward_rows_f64) on top of
tests/lattice64 -- the half stack [ a | a (x) x ], the one-sided reference and the case list of
tests/test_rows_backward_f64_gpu.py.  numpy only: tests/test_rows_backward_f64_host.py uses it without a GPU.

With G the incoming gradient (non-zero on the out rows only) and S the right-hand side (non-zero on the source rows only)
the four terms of py:113-123 split by sides:
    source rows:  -2 sum_l ( s_l x_k wg_l - s_l wgx_lk ),   [ wg | wgx ] = K[src rows, out rows] [ g | g (x) x ]
    out rows:     -2 sum_l ( g_l x_k ws_l - g_l wsx_lk ),   [ ws | wsx ] = K[out rows, src rows] [ s | s (x) x ]
One side is one_sided(a, a_range, b, b_range, x, l64): a the matrix that is filtered, b the one it is contracted against.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -52


def half_stack64(a, x_rows):
    """[ a | a (x) x ] in float64 for a [r, L] and the positions x_rows [r, d] of the same rows: r x L (1 + d), the product
    block l-major (column L + l d + k holds a_l x_k), one multiply per product element."""
    a, x_rows = np.asarray(a, np.float64), np.asarray(x_rows, np.float64)
    r, L = a.shape
    return np.concatenate([a, (a[:, :, None] * x_rows[:, None, :]).reshape(r, L * x_rows.shape[1])], axis=1)


def padded_half_stack64(a, a_range, x):
    """The n-row matrix that holds half_stack64 of the rows [a_begin, a_begin + a_count) and zeros elsewhere."""
    ab, ac = a_range
    assert a.shape[0] == ac
    z = np.zeros((x.shape[0], a.shape[1] * (1 + x.shape[1])))
    z[ab:ab + ac] = half_stack64(a, x[ab:ab + ac])
    return z


def one_sided(a, a_range, b, b_range, x, l64):
    """(want [b_count, d] in longdouble, filtered [b_count, L], T'' [b_count, d], t(a) [b_count, L]):
        want[i][k] = -2 sum_l ( b_l x_k wa_l - b_l wax_lk )          from Lattice64.apply_staged of the padded half stack
        T''[i][k]  =  2 sum_l ( |b_l x_k| t(a)_l + |b_l| t(a (x) x)_lk ),    t(.) = Lattice64.terms64 of it
    at the rows of b; filtered = wa, the float64 filter of a on those rows."""
    (bb, bc), L, d = b_range, a.shape[1], x.shape[1]
    assert b.shape == (bc, L)
    z = padded_half_stack64(a, a_range, x)
    f, t = l64.apply_staged(z)[bb:bb + bc], l64.terms64(z)[bb:bb + bc]
    wa, wax = f[:, :L].astype(LD), f[:, L:].astype(LD).reshape(bc, L, d)
    ta, tax = t[:, :L], t[:, L:].reshape(bc, L, d)
    b3, x3 = b.astype(LD)[:, :, None], x[bb:bb + bc].astype(LD)[:, None, :]
    want = -2 * (b3 * x3 * wa[:, :, None] - b3 * wax).sum(1)
    p3, y3 = np.abs(b)[:, :, None], np.abs(x[bb:bb + bc])[:, None, :]
    T = 2.0 * (p3 * y3 * ta[:, :, None] + p3 * tax).sum(1)
    return want, f[:, :L].copy(), T, ta.copy()


def scatter_sides(n, d, src_range, out_range, grad_src_rows, grad_out_rows):
    """The two one-sided results added into one zero [n, d] matrix (overlapping ranges add up)."""
    out = np.zeros((n, d), dtype=np.result_type(grad_src_rows, grad_out_rows))
    out[src_range[0]:src_range[0] + src_range[1]] += grad_src_rows
    out[out_range[0]:out_range[0] + out_range[1]] += grad_out_rows
    return out


def depth64(l64):
    """k of tests/test_f64_gpu.py from the CPU lattice: the additions and multiplications along the deepest path of the fp64
    product (the longest vertex row, the blur taps of every axis, the slice)."""
    lmax = int(np.diff(l64.S.tocsc().indptr).max())
    d, r = l64.d, l64.coeffs.size // 2
    return lmax + (2 * r + 1) * (d + 1) + 2 * (d + 1) + 8


def chunks(d, L):
    """double2 chunks per vertex row of the half stack: L (1 + d) doubles rounded up to even."""
    return (L * (1 + d) + 1) // 2


# (d, L, derivative-tap order, profile, cloud, buffers 16-byte aligned, range of tests.test_rows_fp64.ranges): the range's
# "source" side is the a range of the first one-sided call, its "output" side the b range; the second call swaps them
CASES = [
    (1, 1, 0, "rbf", "gauss1", True, "head0.8"),           # H = 2, one chunk
    (3, 2, 1, "rbf", "simplex", False, "head0.5T"),        # vertex rows of many corners
    (8, 3, 2, "matern32", "dup", True, "overlap"),         # H = 27, odd: the padding column
    (8, 1, 1, "rbf", "gauss1", False, "oneT"),             # the prediction-mean shape, a one-row range on either side
    (8, 1, 1, "rbf", "gauss1", True, "one"),
    (3, 32, 3, "matern32", "gauss1", False, "head0.8"),    # 64 chunks, the last chunk shape
    (2, 43, 1, "rbf", "gauss1", True, "head0.8T"),         # H = 129, 65 chunks: the first wide shape, with padding
    (4, 26, 1, "rbf", "isolated", True, "equal"),          # 65 chunks, even; rows no term reaches must be exactly 0
    (8, 11, 1, "rbf", "gauss1", False, "head0.8T"),        # the training shape, 50 chunks
    (18, 1, 1, "matern32", "gauss1", True, "head0.5"),     # d = 18, chunk
    (18, 8, 0, "rbf", "gauss1", False, "full"),            # ... and wide; full on both ends
    (24, 1, 2, "rbf", "gauss1", False, "overlap"),         # d + 1 > 20: the run-time form, chunk
    (24, 6, 1, "matern32", "gauss1", True, "head0.5"),     # ... and wide
]
IDS = [f"d{d}-L{L}-o{o}-{p}-{c}-{'al' if a else 'off'}-{r}" for d, L, o, p, c, a, r in CASES]
