"""The fp32 bars of the transposed and the symmetrised lattice products, shown to be satisfiable without a GPU.

tests/sym32.py derives the bars (ENTRY * T_t for K^T v, (ENTRY + 2^-24) * T_s for K_s v, exactly 0 where T is 0) and models
both products in numpy float32 from the data of tests/sym64.Sym64 with EVERY intermediate rounded to float32.  If that
model -- plain fp32 arithmetic in a fixed order, no fused multiply-add -- met the bars with nothing to spare, no kernel
could be held to them; it stays well inside (the worst ratios are printed).
"""
import numpy as np
import pytest

from tests.lattice64 import cloud
from tests.sym32 import ENTRY, ENTRY_SYM, U32, model32, ratios
from tests.sym64 import Sym64, taps_of

N = 300
CASES = [(d, order, lop) for d in (1, 3, 8) for order in (0, 1, 2, 3) for lop in (False, True)]


def test_bars_are_the_forward_bar_and_one_rounding():
    assert ENTRY == 1.8e-6 and U32 == 2.0 ** -24 and ENTRY_SYM == ENTRY + 2.0 ** -24


@pytest.mark.parametrize("d,order,lop", CASES, ids=[f"d{d}-o{o}-{'lop' if l else 'sym'}" for d, o, l in CASES])
def test_fp32_model_meets_the_bars(d, order, lop):
    taps = taps_of(order, lop)
    x = cloud("gauss1", N, d, seed=7 + d + order, coeffs=taps)
    op = Sym64(x, taps)
    v = np.random.default_rng(d * 10 + order).standard_normal((N, 3)).astype(np.float32)
    got_t, got_s = model32(op, v)
    assert got_t.dtype == np.float32 and got_s.dtype == np.float32
    et, es, Tt, Ts = ratios(op, v, got_t, got_s)
    print(f"d = {d} order {order} {'lopsided' if lop else 'symmetric'} taps, m = {op.m}: K^T entry {et:.2e} (bar {ENTRY:.2e}), "
          f"K_s entry {es:.2e} (bar {ENTRY_SYM:.2e})")
    assert et <= ENTRY, (et, ENTRY)
    assert es <= ENTRY_SYM, (es, ENTRY_SYM)


def test_an_entry_no_term_reaches_is_exactly_zero():
    """Isolated points with every other input row zero: T = 0 on those rows, and the fp32 products are exact zeros there
    (entry_ratio returns inf otherwise)."""
    d, order = 3, 1
    taps = taps_of(order, True)
    x = cloud("isolated", N, d, seed=1, coeffs=taps)
    op = Sym64(x, taps)
    v = np.random.default_rng(2).standard_normal((N, 2)).astype(np.float32)
    v[::2] = 0.0
    got_t, got_s = model32(op, v)
    et, es, Tt, Ts = ratios(op, v, got_t, got_s)
    zero = (Tt == 0).all(axis=1) & (Ts == 0).all(axis=1)
    assert zero.sum() >= N // 2 - 1
    assert np.all(got_t[zero] == 0) and np.all(got_s[zero] == 0)
    assert et <= ENTRY and es <= ENTRY_SYM
