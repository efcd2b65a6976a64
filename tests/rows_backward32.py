"""TEST HELPER: the one-sided fp32 position gradient of the rectangular product (plx_apply_backward_rows) -- the count k32 of
its bar and the case list of tests/test_rows_backward_gpu.py, on top of tests/rows_backward64 (one_sided, half_stack64,
scatter_sides, depth64 are reused as they are).  numpy only: tests/test_rows_backward_host.py uses it without a GPU.

k32: the fp32 roundings along the deepest path of the product [ wa | wax ] = K[b rows, a rows] [ a | a (x) x ], counted as
depth64 counts the float64 one (Lmax corners in the longest vertex row, 2 r + 1 taps on each of d + 1 axes, d + 1 corners in
the slice, 8 for the stack multiply, the conversions and slack), with every multiply-add counted as TWO roundings (whether
the compiler fuses it or not), the slice's term carrying the extra multiply by rden = fl(1 / (1 + 2^-d)), and rden's own
rounding:
    splat   2 Lmax                 acc += w * element per corner
    blur    2 (2 r + 1)(d + 1)     a multiply and an addition per tap
    slice   3 (d + 1)              (w * g) * rden, then the addition
    rden    1
    slack   8                      as depth64: the stack multiply a * x, the weights' own roundings
The float64 reference's own error is below 2^-29 of this and is covered by judging against 2^-23 (twice the unit roundoff).
"""
import numpy as np

from tests.rows_backward64 import depth64, half_stack64, one_sided, scatter_sides  # noqa: F401  (re-exported)

U32 = 2.0 ** -23


def k32(l64):
    """The fp32 roundings along the deepest path of the product on this lattice (module docstring)."""
    lmax = int(np.diff(l64.S.tocsc().indptr).max())
    d, r = l64.d, l64.coeffs.size // 2
    return 2 * lmax + 2 * (2 * r + 1) * (d + 1) + 3 * (d + 1) + 1 + 8


def chunks32(d, L):
    """float4 chunks per vertex row of the half stack: L (1 + d) floats rounded up to a multiple of 4."""
    return (L * (1 + d) + 3) // 4


# (d, L, derivative-tap order, profile, cloud, buffers 16-byte aligned, range of tests.test_rows_fp64.ranges): the range's
# "source" side is the a range of the first one-sided call, its "output" side the b range; the second call swaps them
CASES = [
    (1, 1, 0, "rbf", "gauss1", True, "head0.8"),           # H = 2, one chunk, two padding columns
    (8, 1, 1, "rbf", "gauss1", False, "oneT"),             # H = 9, three padding columns: the prediction-mean shape
    (8, 1, 1, "rbf", "gauss1", True, "one"),
    (8, 3, 2, "matern32", "dup", True, "overlap"),         # H = 27, one padding column
    (3, 2, 1, "rbf", "simplex", False, "head0.5T"),        # H = 8: vertex rows of many corners
    (8, 11, 1, "rbf", "gauss1", False, "head0.8T"),        # the training shape, 25 chunks
    (3, 64, 3, "matern32", "gauss1", False, "head0.8"),    # 64 chunks, the last chunk shape
    (5, 43, 1, "rbf", "gauss1", True, "head0.8T"),         # H = 258, 65 chunks: the first wide shape, two padding columns
    (9, 26, 1, "rbf", "isolated", True, "equal"),          # H = 260, 65 chunks, no padding; rows no term reaches are exactly 0
    (18, 1, 1, "matern32", "gauss1", True, "head0.5"),     # d = 18, chunk
    (18, 16, 0, "rbf", "gauss1", False, "full"),           # ... and wide, 76 chunks; full on both ends
    (24, 1, 2, "rbf", "gauss1", False, "overlap"),         # d + 1 > 20: the run-time form, chunk
    (24, 11, 1, "matern32", "gauss1", True, "head0.5"),    # ... and wide, 69 chunks
]
IDS = [f"d{d}-L{L}-o{o}-{p}-{c}-{'al' if a else 'off'}-{r}" for d, L, o, p, c, a, r in CASES]
