"""CPU checks of the transposed / symmetrised float64 lattice products: the identity they rest on, and their declarations.

The GPU forms K^T by running the axes in reverse order with mirrored taps.  That is the transposed matrix only because the
neighbour table of a plain build is symmetric (u is the +j neighbour of v exactly when v is the -j neighbour of u); here the
construction (tests/sym64.transposed64) is compared with the transposed dense matrix of tests/lattice64.Lattice64.

Bar: both matrices sum, entry by entry, the same non-negative products (weights and taps are non-negative) in another
order, so they differ by the rounding of those sums: 8 2^-52 of the entry's terms, which for non-negative terms is the entry
itself.  An entry that no term reaches is exactly 0 on both sides.
"""
import re

import numpy as np
import pytest

from simplex_gp_amd import _native
from tests.lattice64 import cloud
from tests.sym64 import Sym64, taps_of

U2 = 2.0 ** -52

CASES = [(d, order, lop, n)
         for d, n in ((1, 400), (2, 300), (3, 300), (8, 150))
         for order in (0, 1, 2, 3)
         for lop in (False, True)]


@pytest.mark.parametrize("d,order,lop,n", CASES, ids=[f"d{d}-o{o}-{'lop' if l else 'sym'}" for d, o, l, _ in CASES])
def test_reversed_axes_with_mirrored_taps_is_the_transpose(d, order, lop, n):
    taps = taps_of(order, lop)
    assert taps.size == 2 * order + 1 and (taps > 0).all()
    x = cloud("gauss1", n, d, seed=d + order, coeffs=taps)
    op = Sym64(x, taps)
    K, Kt = op.k.matrix(), op.kt.matrix()
    T = K.T                                     # non-negative terms: the size of what an entry sums is the entry
    gap = np.abs(Kt - T)
    print(f"d = {d} order {order} {'lopsided' if lop else 'symmetric'} taps, n = {n}, m = {op.m}: max |Kt64 - K64^T| = "
          f"{gap.max():.2e}, max ratio to the entry {np.max(gap[T > 0] / T[T > 0]):.2e} (bar {8 * U2:.2e})")
    assert np.all(Kt[T == 0] == 0)
    assert np.all(gap <= 8 * U2 * T)
    if lop and order > 0 and d > 1:             # (at d = 1 K came out symmetric to rounding with every tap set here)
        assert np.abs(K - K.T).max() > 1e-3     # the case means something: K itself is far from symmetric
    Ks = op.matrix()
    assert np.all(np.abs(Ks - Ks.T) <= 8 * U2 * Ks)


def test_terms_of_the_symmetrised_operator_bound_it():
    taps = taps_of(2, True)
    x = cloud("gauss1", 200, 3, seed=5, coeffs=taps)
    op = Sym64(x, taps)
    v = np.random.default_rng(0).standard_normal((200, 3))
    assert np.all(np.abs(op.apply_staged(v)) <= op.terms64(v) * (1 + 1e-12))
    assert np.allclose(op.apply_staged(v), op.matrix() @ v, rtol=0, atol=1e-12)


NEW_SYMBOLS = {"plx_blur_t_f64": 6, "plx_apply_t_f64": 5, "plx_blur_sym_work_doubles": 2, "plx_blur_sym_f64": 6,
               "plx_apply_sym_f64": 5, "plx_apply_affine_sym_f64": 8, "plx_last_sym_f64_kernels": 3}


def test_new_symbols_are_declared_with_matching_arity():
    text = re.sub(r"/\*.*?\*/", "", open(_native.HEADER_PATH).read(), flags=re.S)
    declared = _native.declared_symbols()
    for name, arity in NEW_SYMBOLS.items():
        assert name in declared and name in _native._SIGNATURES and name in _native.OPTIONAL_SYMBOLS, name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(_native._SIGNATURES[name][1]), name
    # the affine form takes the argument list of plx_apply_affine_f64
    assert _native._SIGNATURES["plx_apply_affine_sym_f64"] == _native._SIGNATURES["plx_apply_affine_f64"]
    assert _native._SIGNATURES["plx_blur_t_f64"] == _native._SIGNATURES["plx_blur_f64"]
    assert _native.ABI_VERSION == (0, 9)          # detected by symbol: the version string stays
