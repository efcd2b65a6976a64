"""TEST HELPER: every Lattice entry point interleaved on ONE object, each step held to float64 and to a fresh twin.

A plx_lattice keeps tables that their first user builds (one ready flag each), scratch that the table builders share and
value planes that both precisions and six entry points use at different strides (csrc/plx_internal.h).  The per-feature
test modules each run on a lattice of their own; this helper drives all of them through one object, the way
lattice_kernel.py's cached lattice is used by a training step and the evaluation after it:

    scenario   a cloud small enough for a float64 operator and large enough for one lazily chosen path (SCENARIOS)
    chain      five builds on the one object: cold on x, warm on 1.05 x (reuse_order), cold on another cloud (other n, d and
               order-2 lopsided taps), filter_once (the single-use build), cold on x again.  The last segment repeats the
               first segment's calls.
    segment    the ops between two builds; an op is one entry of OPS (one Lattice method, or the few calls that make one
               staged product), its arguments a function of (scenario, build, op) alone
    sequence   a few chains, at most STEP_CAP ops: one pytest case

Per step (check_step): (a) every result against the float64 reference of the op's own test module, under that module's
bar -- nothing here states a bar of its own; (b) the bits and the reported kernel names against a fresh twin that replayed
only the builds since the last cold one and makes this one call; (c) guard elements around every buffer; (d) in the last
segment, the bits of the same call in the first.

The table, the generator and the judges import no GPU code at module import (tests/test_interleave.py runs them without
one); run() and Runner need the GPU.
"""
import ast
import os
import zlib

import numpy as np

from tests.lattice64 import cloud, contract64, entry_ratio, grad_x_ratios, rel_l2, stack64
from tests.sym64 import LOPSIDED

RBF1 = np.array([0.34608543, 1.0, 0.34608543], np.float32)
STEP_CAP = 50
SEGMENT_OPS = 3
U2, U24 = 2.0 ** -52, 2.0 ** -24
LD = np.longdouble
PLX_ERR_STATE = 5                              # plx.h

# name -> cloud of the scenario, the other cloud of build 3 (another n: one larger / one smaller by turns, another d), and
# the regime the shipped switches pick (ISSUE table; the CPU-checkable conditions are in tests/test_interleave.py)
SCENARIOS = {
    "coarse": dict(kind="gauss1", n=600, d=3, other=(601, 5), regime="block"),
    "mid": dict(kind="gauss1", n=500, d=8, other=(499, 3), regime="csr"),
    "fine": dict(kind="gauss3", n=500, d=5, other=(501, 8), regime="first"),
    "fine-large": dict(kind="gauss3", n=2100, d=8, other=(2099, 3), regime="compact"),
    "mid-large": dict(kind="gauss1", n=3200, d=8, other=(3201, 5), regime="pair"),
}
BACKWARD_NRHS = {3: 16, 5: 11, 8: 7}          # Lattice.backward_fusable holds (tests/test_interleave.py)
F64_NRHS = 3
ROWS_NRHS = 3
CYCLE = ("head", "overlap", "equal", "head")  # five distinct row ranges, one more than plx_lattice::kRowsRanges, then the first

BUILDS = ("cold", "warm", "other", "once", "again")
BUILD_KIND = {"cold": "cold", "warm": "warm", "other": "cold", "once": "once", "again": "cold"}
KINDS = ("cold", "warm", "once")
GROUPS = tuple(f"G{i}" for i in range(1, 15))
ROW_ORDER_GROUPS = ("G1", "G2", "G3")         # the ops that follow set_lattice_row_order

# (earlier op, op) -> the source line that makes the dependence of `op`'s bits or kernel family on `earlier op` intended.
# No op for which plx.h states a bit contract may appear.  Empty: no dependence is known or tolerated.
INTENDED_DEPENDENCE = {}


# ---- the op table -----------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, group, methods, run, judge, **kw):
        self.name, self.group, self.methods, self.run, self.judge, self.kw = name, group, tuple(methods), run, judge, kw


OPS = {}


def op(name, group, methods, run, judge, **kw):
    assert name not in OPS
    OPS[name] = Op(name, group, methods, run, judge, **kw)


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- references: one per build of the chain, from the CPU oracle alone ---------------------------------------------------
class Ref:
    """The positions and taps of one build, and every float64 operator on them, each formed once."""

    def __init__(self, tag, x, taps):
        self.tag, self.x, self.taps = tag, np.ascontiguousarray(x, np.float32), np.ascontiguousarray(taps, np.float32)
        self.n, self.d = self.x.shape
        self.order = self.taps.size // 2
        self._sym = self._q = self._diag = self._depth = self._x64 = None
        self.memo = {}

    @property
    def sym(self):
        if self._sym is None:
            from tests.sym64 import Sym64
            self._sym = Sym64(self.x, self.taps)
        return self._sym

    @property
    def l64(self):
        return self.sym.k

    @property
    def depth(self):
        """k of tests/test_f64_gpu.py, from the CPU lattice (tests/rows_backward64.depth64: no export on the object)."""
        if self._depth is None:
            from tests.rows_backward64 import depth64
            self._depth = depth64(self.l64)
        return self._depth

    def rhs(self, tag, rows, vd, dtype=np.float32):
        return np.random.default_rng(seed_of(self.tag, tag)).standard_normal((rows, vd)).astype(dtype)

    @property
    def x64(self):
        """float64 positions that round to x and differ from it in the low bits (tests/test_backward_f64_gpu.positions64)."""
        if self._x64 is None:
            rng = np.random.default_rng(seed_of(self.tag, "x64"))
            x = self.x.astype(np.float64) * (1.0 + 1e-9 * rng.standard_normal(self.x.shape))
            assert np.array_equal(x.astype(np.float32), self.x)
            self._x64 = x
        return self._x64

    def queries(self):
        """100 build points, 100 jittered points, 20 far away (tests/test_query_gpu.queries)."""
        from oracle import oracle
        rng = np.random.default_rng(seed_of(self.tag, "queries"))
        x, d = self.x, self.d
        train = x[rng.permutation(self.n)[:100]]
        jit = (x[:100] + 0.05 * rng.standard_normal((100, d))).astype(np.float32)
        far = x[:20].copy()
        far[:, 0] += np.float32(x[:, 0].max() - x[:, 0].min() + 12.0 * d / float(oracle.scale_factors(d, self.taps)[0]))
        return np.ascontiguousarray(np.concatenate([train, jit, far], 0), np.float32)

    @property
    def q64(self):
        if self._q is None:
            from tests.query64 import Query64
            self._q = Query64(self.x, self.queries(), self.taps, lattice=self.l64)
        return self._q

    @property
    def diag(self):
        if self._diag is None:
            from tests import diag64
            self._diag = (diag64.diag_dense(self.l64), diag64.diag_terms(self.l64), diag64.bar_terms(self.d, self.order))
        return self._diag

    def cached(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]


_REFS = {}


def refs(scn):
    """{build name: Ref} of a scenario's chain ("again" is "cold": the same cloud)."""
    if scn not in _REFS:
        s = SCENARIOS[scn]
        x = cloud(s["kind"], s["n"], s["d"], seed=1, coeffs=RBF1)
        n2, d2 = s["other"]
        taps2 = LOPSIDED[2]
        cold = Ref((scn, "cold"), x, RBF1)
        _REFS[scn] = {"cold": cold, "warm": Ref((scn, "warm"), x * np.float32(1.05), RBF1),
                      "other": Ref((scn, "other"), cloud("gauss1", n2, d2, seed=2, coeffs=taps2), taps2),
                      "once": Ref((scn, "once"), x * np.float32(0.9), RBF1), "again": cold}
    return _REFS[scn]


# ---- the judges: check items from a reference and the device results (numpy) ---------------------------------------------
# An item is (label, ratio to its bar): the step passes when every ratio is <= 1.  A result that is not finite, or that is
# not exactly 0 where no term reaches it, has ratio inf (lattice64.entry_ratio).
def item_entry(label, got, want, T, bar, rel_bar=None):
    out = [(label + " entry", entry_ratio(got, want, T) / bar)]
    if rel_bar is not None and np.linalg.norm(want) > 0:
        out.append((label + " rel-L2", rel_l2(got, want) / rel_bar))
    return out


def item_ratio(label, got, want, T, bar):
    """tests/test_backward_f64_gpu.ratio_to_bar: the error in longdouble against bar * T, every entry."""
    from tests.test_backward_f64_gpu import ratio_to_bar
    return [(label, ratio_to_bar(np.asarray(got), np.asarray(want, LD), np.asarray(T), bar, label))]


def item_equal(label, got, want):
    return [(label + " exact", 0.0 if np.array_equal(np.asarray(got), np.asarray(want)) else float("inf"))]


def forward_bars():
    from tests.test_forward_fp64 import DOT, ENTRY, REL
    return ENTRY, REL, DOT


def fwd_reference(ref, v):
    return ref.l64.apply_staged(v), ref.l64.terms64(v)


def judge_forward(ref, res, tag, vd, **kw):
    """fp32 K v (apply, the stages, one-hot columns): ENTRY and REL of tests/test_forward_fp64."""
    ENTRY, REL, _ = forward_bars()
    v = ref.rhs(tag, ref.n, vd)
    want, T = ref.cached(("fwd", tag, vd), lambda: fwd_reference(ref, v))
    return item_entry("out", res["out"], want, T, ENTRY, REL)


def judge_affine(ref, res, tag, vd, dot=None, **kw):
    ENTRY, REL, DOT = forward_bars()
    v = ref.rhs(tag, ref.n, vd)
    kv, T = ref.cached(("fwd", tag, vd), lambda: fwd_reference(ref, v))
    a, b = AFFINE
    want, T = a * kv + b * v, abs(a) * T + abs(b) * np.abs(v)
    items = item_entry("out", res["out"], want, T, ENTRY, REL)
    if dot:
        dwant, dterms = (v.astype(np.float64) * want).sum(0), (np.abs(v) * np.abs(want)).sum(0)
        items.append(("dot", float(np.max(np.abs(np.asarray(res["dot"], np.float64) - dwant) / dterms)) / DOT))
    return items


def judge_backward32(ref, res, **kw):
    from tests.test_backward_fp64 import REL, REL_X, TAU
    L = BACKWARD_NRHS[ref.d]
    g, s = ref.rhs("bwd32 g", ref.n, L), ref.rhs("bwd32 s", ref.n, L)
    gx64, gs64, T = ref.cached("bwd32", lambda: contract64(g, s, ref.x, ref.l64.apply_staged(stack64(g, s, ref.x))))
    terms, rel = grad_x_ratios(res["grad_x"], gx64, T)
    items = [("grad_x / ||T||", terms / TAU), ("grad_src rel-L2", rel_l2(res["grad_src"], gs64) / REL)]
    if rel is not None:
        items.append(("grad_x rel-L2", rel / REL_X))
    if not np.all(np.isfinite(res["grad_x"])):
        items.append(("grad_x finite", float("inf")))
    return items


def rows_ranges(rname, n):
    from tests.test_rows_fp64 import ranges
    return ranges({"head": "head0.8", "tail": "head0.8T", "overlap": "overlap", "full": "full", "equal": "equal"}[rname], n)


def padded_rows(ref, tag, rname, vd, dtype):
    (sb, sc), (ob, oc) = rows_ranges(rname, ref.n)
    v = ref.rhs(tag, sc, vd, dtype)
    padded = np.zeros((ref.n, vd), dtype)
    padded[sb:sb + sc] = v
    return v, padded, (sb, sc), (ob, oc)


def judge_rows32(ref, res, tag, rname, vd, **kw):
    from tests.test_rows_fp64 import ENTRY, REL
    _, padded, _, (ob, oc) = padded_rows(ref, tag, rname, vd, np.float32)
    want, T = ref.cached(("rows", tag, rname, vd), lambda: tuple(a[ob:ob + oc] for a in fwd_reference(ref, padded)))
    return item_entry("out", res["out"], want, T, ENTRY, REL)


def judge_f64(ref, res, want, T, extra=0):
    """tests/test_f64_gpu.check64: per entry k 2^-52 of T, rel-L2 k 2^-52 ||T|| / ||want||."""
    k = ref.depth + extra
    rbar = k * U2 * float(np.linalg.norm(T)) / max(float(np.linalg.norm(want)), 1e-300)
    return item_entry("out", res["out"], want, T, k * U2, rbar if rbar > 0 else None)


def judge_rows64(ref, res, tag, rname, vd, **kw):
    _, padded, _, (ob, oc) = padded_rows(ref, tag, rname, vd, np.float64)
    want, T = ref.cached(("rows", tag, rname, vd), lambda: tuple(a[ob:ob + oc] for a in fwd_reference(ref, padded)))
    return judge_f64(ref, res, want, T)


def judge_rows_cycle(ref, res, tag, vd, f64=False, **kw):
    items = []
    for i, rname in enumerate(CYCLE):
        one = (judge_rows64 if f64 else judge_rows32)(ref, {"out": res[f"out{i}"]}, tag + rname, rname, vd)
        items += [(f"{rname}[{i}] {label}", ratio) for label, ratio in one]
    return items + item_equal("the first range again", res["out3"], res["out0"])


def backward_rows_inputs(ref, dtype):
    (ab, ac), (bb, bc) = rows_ranges("overlap", ref.n)
    a, b = ref.rhs(("bwdrows a", str(dtype)), ac, ROWS_NRHS, dtype), ref.rhs(("bwdrows b", str(dtype)), bc, ROWS_NRHS, dtype)
    x = ref.x if dtype == np.float32 else ref.x64
    return a, (ab, ac), b, (bb, bc), x


def judge_backward_rows(ref, res, f64, **kw):
    from tests import rows_backward32, rows_backward64
    a, a_rng, b, b_rng, x = backward_rows_inputs(ref, np.float64 if f64 else np.float32)
    want, filt, T, ta = ref.cached(("bwdrows", f64), lambda: rows_backward64.one_sided(
        a.astype(np.float64), a_rng, b.astype(np.float64), b_rng, x.astype(np.float64), ref.l64))
    L = ROWS_NRHS
    if f64:           # tests/test_rows_backward_f64_gpu.py
        k = ref.depth
        bar_x, bar_f = 2 * (k + 2 * (L + 1)) * U2, k * U2
    else:             # tests/test_rows_backward_gpu.py
        k = rows_backward32.k32(ref.l64)
        bar_x, bar_f = (k + 2 * (L + 1)) * rows_backward32.U32, k * rows_backward32.U32
    return item_ratio("grad_x", res["grad_x"], want, T, bar_x) + item_ratio("filtered", res["filtered"], filt, ta, bar_f)


def judge_sym32(ref, res, tag, vd, which, dot=False, **kw):
    """tests/sym32: K^T under ENTRY of its terms, K_s under ENTRY + 2^-24."""
    from tests import sym32
    v = ref.rhs(tag, ref.n, vd)
    v64 = v.astype(np.float64)
    op64, bar = (ref.sym.kt, sym32.ENTRY) if which == "t" else (ref.sym, sym32.ENTRY_SYM)
    want, T = ref.cached(("sym32", tag, vd, which), lambda: (op64.apply_staged(v64), op64.terms64(v64)))   # sym32.ratios
    items = item_entry("out", res["out"], want, T, bar)
    if dot:           # tests/test_sym_gpu.py: n products summed in fp32 in a fixed order
        out64 = np.asarray(res["out"], np.float64)
        exact, terms = (v.astype(np.float64) * out64).sum(0), np.abs(v.astype(np.float64) * out64).sum(0)
        items.append(("dot", float(np.max(np.abs(np.asarray(res["dot"], np.float64) - exact) / terms)) / ((ref.n + 4) * sym32.U32)))
    return items


def judge_apply64(ref, res, tag, vd, **kw):
    v = ref.rhs(tag, ref.n, vd, np.float64)
    want, T = ref.cached(("fwd64", tag, vd), lambda: fwd_reference(ref, v))
    return judge_f64(ref, res, want, T)


def dot64_items(ref, v, res):
    """tests/test_cg_f64_gpu.py: the fused dot against the longdouble dot of src and the returned out, (n + 4) 2^-52."""
    g = np.asarray(res["out"], np.float64)
    wdot, tdot = (v.astype(LD) * g.astype(LD)).sum(0), np.abs(v * g).sum(0)
    return [("dot", entry_ratio(res["dot"], np.asarray(wdot, np.float64), tdot) / ((ref.n + 4) * U2))]


def judge_affine64(ref, res, tag, vd, dot=False, **kw):
    v = ref.rhs(tag, ref.n, vd, np.float64)
    kv, T = ref.cached(("fwd64", tag, vd), lambda: fwd_reference(ref, v))
    a, b = AFFINE
    want = np.asarray(LD(a) * np.asarray(kv, LD) + LD(b) * np.asarray(v, LD), np.float64)
    items = item_entry("out", res["out"], want, abs(a) * T + abs(b) * np.abs(v), (ref.depth + 2) * U2)
    return items + (dot64_items(ref, v, res) if dot else [])


def judge_backward64(ref, res, **kw):
    from tests.test_backward_f64_gpu import reference
    L = F64_NRHS
    g, s = ref.rhs("bwd64 g", ref.n, L, np.float64), ref.rhs("bwd64 s", ref.n, L, np.float64)
    want, want_gs, T, tg = ref.cached("bwd64", lambda: reference(g, s, ref.x64, ref.l64))
    k = ref.depth
    return (item_ratio("grad_x", res["grad_x"], want, T, 2 * (k + 4 * (L + 1)) * U2)
            + item_ratio("grad_src", res["grad_src"], want_gs, tg, k * U2))


def judge_sym64(ref, res, tag, vd, which, dot=False, **kw):
    """tests/test_sym_f64_gpu.check_entries: K^T under k 2^-52, K_s under (k + 2) 2^-52."""
    v = ref.rhs(tag, ref.n, vd, np.float64)
    op64, k = (ref.sym.kt, ref.depth) if which == "t" else (ref.sym, ref.depth + 2)
    want, T = ref.cached(("sym64", tag, vd, which), lambda: (op64.apply_staged(v), op64.terms64(v)))
    items = item_entry("out", res["out"], want, T, k * U2)
    return items + (dot64_items(ref, v, res) if dot else [])


def judge_diag(ref, res, f64, rows=None, lattice_rows=False, **kw):
    dense, terms, k = ref.diag
    got = np.asarray(res["out"], np.float64)
    if rows is not None:
        b, c = rows(ref.n)
        dense, terms = dense[b:b + c], terms[b:b + c]
    if lattice_rows:
        perm = np.asarray(res["perm"], np.int64)
        dense, terms = dense[perm], terms[perm]
    return item_entry("diag", got, dense, terms, k * (U2 if f64 else U24))


def judge_query(ref, res, f64, vd, **kw):
    """tests/test_query_gpu.py: locate exact; apply_at float64 under k 2^-52 of its terms, fp32 under ENTRY / REL."""
    ENTRY, REL, _ = forward_bars()
    if "refused" in res:          # the single-use build: the refusal wrote nothing
        return [("refusal leaves vid alone exact", 0.0 if not np.asarray(res["vid"]).any() else float("inf"))]
    q = ref.q64
    vid = np.asarray(res["vid"], np.int64).T
    items = item_equal("found", vid >= 0, q.found)
    if vid.shape == q.found.shape and np.array_equal(vid >= 0, q.found):
        keys = np.asarray(res["keys"])
        ok = vid.max() < keys.shape[0] and np.array_equal(keys[vid[q.found]], q.qkeys[q.found])
        items.append(("keys of the found ids exact", 0.0 if ok else float("inf")))
    items += item_equal("weight", np.asarray(res["weight"]).T, q.weight) + item_equal("mass", res["mass"], q.mass32)
    v = ref.rhs(("query", f64), ref.n, vd, np.float64 if f64 else np.float32)
    want, T = ref.cached(("query", f64, vd), lambda: (q.apply64(v), q.terms64(v)))
    if f64:
        return items + item_entry("out", res["out"], want, T, ref.depth * U2)
    return items + item_entry("out", res["out"], want, T, ENTRY, REL)


def onehot_points(ref, tag, nb):
    pts = np.random.default_rng(seed_of(ref.tag, tag)).choice(ref.n, nb, replace=False).astype(np.int32)
    if nb >= 3:
        pts[1], pts[2] = (pts[0] + 1) % ref.n, pts[0]          # neighbours in lattice order; the same point twice
    return pts


def judge_onehot(ref, res, tag, vd, nb, **kw):
    ENTRY, REL, _ = forward_bars()
    cols = np.asarray(res["perm"], np.int64)[onehot_points(ref, tag, nb)]
    e = np.zeros((ref.n, vd), np.float32)
    e[cols, np.arange(nb)] = 1.0
    want, T = fwd_reference(ref, e)
    return item_entry("out", res["out"], want, T, ENTRY, REL)


def judge_nothing(ref, res, **kw):
    return []


AFFINE = (0.9, 0.35)


# ---- the step checker --------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def values_equal(a, b):
    """torch.equal on numpy arrays: the same shape and every element equal as a value (NaN equals nothing)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(a == b))


def check_step(opname, ref, res, twin=None, kernels=None, twin_kernels=None, first=None, earlier=None, label=""):
    """The verdict on one step.  res / twin / first: {name: numpy array} of this call, of the twin's call and of the same
    call in the chain's first segment; kernels / twin_kernels: what the kernel-name getters reported.  Returns the items
    [(label, ratio to its bar)]; raises AssertionError naming the first contract broken."""
    o = OPS[opname]
    items = o.judge(ref, res, **o.kw)
    for name, ratio in items:
        assert ratio <= 1.0, (label, opname, "float64 bar", name, "ratio to the bar", ratio)
    tolerated = (earlier, opname) in INTENDED_DEPENDENCE
    if twin is not None and not tolerated:
        assert set(twin) == set(res), (label, opname, "the twin returned other arrays")
        for name in res:
            assert values_equal(res[name], twin[name]), (label, opname, "differs from the fresh twin in", name, "after", earlier)
        assert kernels == twin_kernels, (label, opname, "kernel families differ from the twin's", kernels, twin_kernels,
                                         "after", earlier)
    if first is not None:
        for name in res:
            assert values_equal(res[name], first[name]), (label, opname, "the revisit differs from the first segment in", name)
    return items


# ---- the generator -----------------------------------------------------------------------------------------------------
def sequences(scn):
    """The sequences of a scenario: [[chain, ...], ...], chain = [[op name, ...] per build of BUILDS].  Deterministic.
    Every op opens a segment after a cold build, after the warm rebuild and after filter_once; every ordered pair of groups
    is adjacent inside a segment; "row_order" is always followed by an op of G1..G3; the last segment copies the first."""
    rng = np.random.default_rng(seed_of("interleave", scn))
    names = sorted(OPS)
    by_group = {g: [n for n in names if OPS[n].group == g] for g in GROUPS}
    firsts = {k: [names[i] for i in rng.permutation(len(names))] for k in KINDS}
    pairs = {(a, b) for a in GROUPS for b in GROUPS}
    plain = [n for n in names if OPS[n].group in ROW_ORDER_GROUPS]

    def pick(group):
        return by_group[group][int(rng.integers(len(by_group[group])))]

    def segment(kind):
        seg = [firsts[kind].pop() if firsts[kind] else names[int(rng.integers(len(names)))]]
        while len(seg) < SEGMENT_OPS or seg[-1] == "row_order":
            prev = OPS[seg[-1]].group
            if seg[-1] == "row_order":
                wanted = [g for g in ROW_ORDER_GROUPS if (prev, g) in pairs]
                nxt = pick(wanted[int(rng.integers(len(wanted)))]) if wanted else plain[int(rng.integers(len(plain)))]
            else:
                wanted = [g for g in GROUPS if (prev, g) in pairs]
                if not wanted:       # nothing left from here: go where something is
                    wanted = sorted({a for a, _ in pairs}) or list(GROUPS)
                nxt = pick(wanted[int(rng.integers(len(wanted)))])
            pairs.discard((prev, OPS[nxt].group))
            seg.append(nxt)
        return seg

    chains = []
    while any(firsts.values()) or pairs:
        assert len(chains) < 4 * len(names), "the generator does not converge"
        chain = [segment(BUILD_KIND[b]) for b in BUILDS[:4]]
        chains.append(chain + [list(chain[0])])
    seqs, cur, steps = [], [], 0
    for chain in chains:
        k = sum(len(s) for s in chain)
        if cur and steps + k > STEP_CAP:
            seqs.append(cur)
            cur, steps = [], 0
        cur.append(chain)
        steps += k
    if cur:
        seqs.append(cur)
    return seqs


def steps_of(seq):
    """[(chain index, build name, position in segment, op name, previous op or None)] of a sequence."""
    return [(ci, b, i, name, seg[i - 1] if i else None)
            for ci, chain in enumerate(seq) for b, seg in zip(BUILDS, chain) for i, name in enumerate(seg)]


# ---- which Lattice methods launch work (from the source) ---------------------------------------------------------------
EXCLUDED_METHODS = {"build_local", "build_merge"}          # sharded builds: the newer entry points refuse them
BUILD_METHODS = {"build", "filter_once"}                   # the chain itself


def launching_methods():
    """The public methods of simplex_gp_amd.lattice.Lattice that reach a plx_* call which takes a stream (a launch),
    directly or through other methods of the class: parsed from the source."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplex_gp_amd", "lattice.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Lattice")
    direct, calls = set(), {}
    for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
        src_names = {n.id for n in ast.walk(fn) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute)}
        strings = {n.value for n in ast.walk(fn) if isinstance(n, ast.Constant) and isinstance(n.value, str)}
        plx = any(s.startswith("plx_") for s in src_names | strings)
        if plx and "_stream_ptr" in src_names:
            direct.add(fn.name)
        calls[fn.name] = {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
                          and n.value.id == "self"}
    reach = set(direct)
    while True:
        more = {f for f, c in calls.items() if f not in reach and c & reach}
        if not more:
            break
        reach |= more
    return {f for f in reach if not f.startswith("_")}


# ---- running on the GPU ------------------------------------------------------------------------------------------------
class Call:
    """The buffers of one op on one lattice: every array in a tests/gpubuf.Buf."""

    def __init__(self, lat, ref, off, lattice_rows=False):
        self.lat, self.ref, self.off, self.lattice_rows = lat, ref, off, lattice_rows
        self.single_use = False
        self.inputs, self.outputs = [], []

    def inp(self, a, dtype=None, aligned=False):
        import torch
        from tests.gpubuf import Buf
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a))
        b = Buf(a, offset=0 if aligned else self.off, dtype=dtype or a.dtype)
        self.inputs.append(b)
        return b.view.view(tuple(a.shape))

    def out(self, shape, dtype, aligned=False):
        from tests.gpubuf import SENTINEL, Buf
        count = int(np.prod(shape))
        b = Buf(count=count, offset=0 if aligned else self.off, dtype=dtype, fill=SENTINEL if dtype.is_floating_point else 0)
        self.outputs.append(b)
        return b.view.view(tuple(shape))

    def values(self, vd, dtype):
        """A vertex plane [m, values_stride(vd)] (16-byte aligned, as Lattice.new_values gives it)."""
        return self.out((self.lat.m, self.lat.values_stride(vd, dtype)), dtype, aligned=True)

    def check(self):
        from tests.gpubuf import check_buffers
        check_buffers(inputs=self.inputs, outputs=self.outputs)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _stream():
    import ctypes
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _fam(d, *keys):
    return {k: list(d.get(k, [])) for k in keys}


def _rows_in(c, v):
    """The rows of the caller's matrix `v` as the lattice takes them (lattice order after set_lattice_row_order)."""
    import torch
    if not c.lattice_rows:
        return c.inp(v)
    c.lat.set_lattice_row_order(True)
    return c.inp(c.lat.to_lattice_order(torch.from_numpy(v).cuda()))


def _rows_out(c, out):
    if not c.lattice_rows:
        return _np(out)
    res = _np(c.lat.from_lattice_order(out))
    c.lat.set_lattice_row_order(False)
    return res


def run_forward(c, tag, vd, mode="apply", **kw):
    import torch
    lat, ref = c.lat, c.ref
    v = ref.rhs(tag, ref.n, vd)
    src, out = _rows_in(c, v), c.out((ref.n, vd), torch.float32)
    res = {}
    if mode == "apply":
        lat.apply(src, out=out)
    elif mode == "stages":
        values, scratch = c.values(vd, torch.float32), c.values(vd, torch.float32)
        lat.splat(src, values)
        lat.slice(lat.blur(values, scratch, vd=vd), out, vd=vd)
    else:
        ss = c.inp(np.array(AFFINE, np.float32), aligned=True)
        if mode == "affine":
            lat.apply_affine(src, ss, out=out)
        elif mode == "dot":
            _, dot = lat.apply_affine(src, ss, out=out, want_dot=True)
            res["dot"] = _np(dot)
        else:
            _, work, tiles = lat.apply_affine(src, ss, out=out, want_dot="partial")
            vdp = lat.values_stride(vd)
            part = work[:tiles * vdp].view(tiles, vdp)
            res["partials"] = _np(part)
            res["dot"] = _np(part).astype(np.float64).sum(0)[:vd]
    kern = _fam(lat.stage_kernels(), "splat", "blur_axis", "slice")
    res["out"] = _rows_out(c, out)
    return res, kern


def run_backward32(c, **kw):
    import torch
    from simplex_gp_amd import _native as nv
    lat, ref = c.lat, c.ref
    L = BACKWARD_NRHS[ref.d]
    assert lat.backward_fusable(L, ref.d)
    g, s, x = c.inp(ref.rhs("bwd32 g", ref.n, L)), c.inp(ref.rhs("bwd32 s", ref.n, L)), c.inp(ref.x)
    gx, gs = c.out((ref.n, ref.d), torch.float32), c.out((ref.n, L), torch.float32)
    with torch.cuda.device(lat.device):
        nv.check(nv.lib().plx_apply_backward(lat._h, _ptr(g), _ptr(s), _ptr(x), L, _ptr(gx), _ptr(gs), _stream()),
                 "plx_apply_backward")
    return {"grad_x": _np(gx), "grad_src": _np(gs)}, _fam(lat.stage_kernels(), "splat", "blur_axis")


def run_rows(c, tag, rname, vd, f64=False, staged=False, **kw):
    import torch
    lat, ref = c.lat, c.ref
    dt, npdt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
    v, _, (sb, sc), (ob, oc) = padded_rows(ref, tag, rname, vd, npdt)
    src, out = c.inp(v), c.out((oc, vd), dt)
    if staged:
        values, scratch = c.values(vd, dt), c.values(vd, dt)
        lat.splat_rows(src, sb, values)
        lat.slice_rows(lat.blur(values, scratch, vd=vd), ob, oc, out=out, vd=vd)
    else:
        lat.apply_rows(src, sb, ob, oc, out=out)
    if f64:
        kern = dict(_fam(lat.rows_f64_kernels(), "splat", "slice"), **_fam(lat.f64_kernels(), "blur_axis"))
    else:
        kern = dict(_fam(lat.rows_kernels(), "splat", "slice"), **_fam(lat.stage_kernels(), "blur_axis"))
    return {"out": _np(out)}, kern


def run_rows_cycle(c, tag, vd, f64=False, **kw):
    """apply_rows over more ranges than the lattice has range slots, then the first again: its tables were recycled."""
    res, kern = {}, {}
    for i, rname in enumerate(CYCLE):
        r, kern = run_rows(c, tag + rname, rname, vd, f64=f64)
        res[f"out{i}"] = r["out"]
    return res, kern


def run_backward_rows(c, f64, **kw):
    import torch
    from simplex_gp_amd import _native as nv
    lat, ref = c.lat, c.ref
    dt, npdt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
    ok = lat.backward_rows_f64_ok if f64 else lat.backward_rows_ok
    assert ok(ROWS_NRHS, ref.d)
    a, (ab, ac), b, (bb, bc), x = backward_rows_inputs(ref, npdt)
    ta, tb, tx = c.inp(a), c.inp(b), c.inp(x)
    gx, filt = c.out((bc, ref.d), dt), c.out((bc, ROWS_NRHS), dt)
    name = "plx_apply_backward_rows_f64" if f64 else "plx_apply_backward_rows"
    with torch.cuda.device(lat.device):
        nv.check(getattr(nv.lib(), name)(lat._h, _ptr(ta), ab, ac, _ptr(tb), bb, bc, _ptr(tx), ROWS_NRHS, _ptr(gx), _ptr(filt),
                                         _stream()), name)
    kern = _fam(lat.rows_f64_kernels() if f64 else lat.rows_kernels(), "splat", "slice")
    return {"grad_x": _np(gx), "filtered": _np(filt)}, kern


def run_sym(c, tag, vd, which, f64=False, mode="apply", dot=False, **kw):
    import torch
    from simplex_gp_amd import _native as nv
    lat, ref = c.lat, c.ref
    dt, npdt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
    src, out = c.inp(ref.rhs(tag, ref.n, vd, npdt)), c.out((ref.n, vd), dt)
    res = {}
    if mode == "apply":
        fn = {("t", False): lat.apply_t_f32, ("s", False): lat.apply_sym_f32, ("t", True): lat.apply_t, ("s", True): lat.apply_sym}
        fn[which, f64](src, out=out)
    elif mode == "affine":     # scale_shift (1, 0): held to the bar of the plain symmetrised product
        ss = c.inp(np.array([1.0, 0.0], npdt), aligned=True)
        if f64:
            _, d_ = lat.apply_affine(src, ss, out=out, want_dot=True, symmetric=True)
        else:
            _, d_ = lat.apply_affine_sym_f32(src, ss, out=out, want_dot=True)
        res["dot"] = _np(d_)
    else:                      # the stages: splat, blur_t / blur_sym, slice
        values = c.values(vd, dt)
        lat.splat(src, values)
        if which == "t":
            scratch = c.values(vd, dt)
            b = (lat.blur_t if f64 else lat.blur_t_f32)(values, scratch, vd=vd)
        else:
            need = int((nv.lib().plx_blur_sym_work_doubles if f64 else nv.lib().plx_blur_sym_work_floats)(lat._h, vd))
            work = c.out((need,), dt, aligned=True)
            b = (lat.blur_sym if f64 else lat.blur_sym_f32)(values, work, vd=vd)
        lat.slice(b.contiguous(), out, vd=vd)
    res["out"] = _np(out)
    return res, _fam(lat.sym_f64_kernels() if f64 else lat.sym_kernels_f32(), "splat", "blur", "slice")


def run_apply64(c, tag, vd, mode="apply", **kw):
    import torch
    lat, ref = c.lat, c.ref
    src, out = c.inp(ref.rhs(tag, ref.n, vd, np.float64)), c.out((ref.n, vd), torch.float64)
    res = {}
    if mode == "apply":
        lat.apply(src, out=out)
    else:
        ss = c.inp(np.array(AFFINE, np.float64), aligned=True)
        if mode == "dot":
            _, d_ = lat.apply_affine(src, ss, out=out, want_dot=True)
            res["dot"] = _np(d_)
        else:
            lat.apply_affine(src, ss, out=out)
    res["out"] = _np(out)
    return res, _fam(lat.f64_kernels(), "splat", "blur_axis", "slice")


def run_backward64(c, **kw):
    import torch
    from simplex_gp_amd import _native as nv
    lat, ref = c.lat, c.ref
    L = F64_NRHS
    assert lat.backward_f64_ok(L, ref.d)
    g, s = c.inp(ref.rhs("bwd64 g", ref.n, L, np.float64)), c.inp(ref.rhs("bwd64 s", ref.n, L, np.float64))
    x = c.inp(ref.x64)
    gx, gs = c.out((ref.n, ref.d), torch.float64), c.out((ref.n, L), torch.float64)
    with torch.cuda.device(lat.device):
        nv.check(nv.lib().plx_apply_backward_f64(lat._h, _ptr(g), _ptr(s), _ptr(x), L, _ptr(gx), _ptr(gs), _stream()),
                 "plx_apply_backward_f64")
    return {"grad_x": _np(gx), "grad_src": _np(gs)}, _fam(lat.f64_kernels(), "splat", "blur_axis", "slice")


def run_diag(c, f64, rows=None, lattice_rows=False, **kw):
    import torch
    lat, ref = c.lat, c.ref
    dt = torch.float64 if f64 else torch.float32
    rng = rows(ref.n) if rows is not None else None
    out = c.out((rng[1] if rng else ref.n,), dt, aligned=True)
    lat.diag(dtype=dt, rows=rng, lattice_rows=lattice_rows, out=out)
    res = {"out": _np(out)}
    if lattice_rows:
        res["perm"] = _np(lat.shard_perm())
    return res, {}


def run_query(c, f64, vd, keys=None, **kw):
    import torch
    from simplex_gp_amd import _native as nv
    from simplex_gp_amd.lattice import LatticeQuery
    lat, ref = c.lat, c.ref
    dt, npdt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
    xq = c.inp(ref.queries(), aligned=True)
    nq, d1 = xq.shape[0], ref.d + 1
    vid, weight = c.out((d1, nq), torch.int32, aligned=True), c.out((d1, nq), torch.float32, aligned=True)
    mass = c.out((nq,), torch.float32, aligned=True)
    with torch.cuda.device(lat.device):
        rc = nv.lib().plx_locate(lat._h, _ptr(xq), nq, _ptr(vid), _ptr(weight), _ptr(mass), _stream())
    if c.single_use:
        # plx_api.hip (query_guard): a lattice built by plx_filter serves one product and refuses queries, before any launch
        assert rc == PLX_ERR_STATE and b"plx_filter" in nv.lib().plx_last_error(), (rc, nv.lib().plx_last_error())
        return {"refused": np.array([rc]), "vid": _np(vid)}, {}
    nv.check(rc, "plx_locate")
    q = LatticeQuery(vid, weight, mass, nq, lat.build_id)
    src = c.inp(ref.rhs(("query", f64), ref.n, vd, npdt))
    values, scratch, out = c.values(vd, dt), c.values(vd, dt), c.out((nq, vd), dt)
    lat.splat(src, values)
    lat.slice_at(lat.blur(values, scratch, vd=vd), q, out=out, vd=vd)
    res = {"vid": _np(vid), "weight": _np(weight), "mass": _np(mass), "out": _np(out), "keys": keys}
    return res, _fam(lat.query_kernels(), "locate", "slice_at")


def run_onehot(c, tag, vd, nb, mode, **kw):
    import torch
    lat, ref = c.lat, c.ref
    pts = c.inp(onehot_points(ref, tag, nb), aligned=True)
    out = c.out((ref.n, vd), torch.float32, aligned=True)
    values, scratch = c.values(vd, torch.float32), c.values(vd, torch.float32)
    if mode == "splat":
        lat.splat_onehot(pts, nb, values, vd=vd)
        lat.slice(lat.blur(values, scratch, vd=vd), out, vd=vd)
    else:
        lat.filter_onehot(pts, nb, values, scratch, out, vd=vd, sparse=(mode == "sparse"))
    kern = _fam(lat.stage_kernels(), "splat", "blur_axis", "slice")
    return {"out": _np(out), "perm": _np(lat.shard_perm())}, kern


def run_prepare(c, vd, **kw):
    c.lat.prepare(vd)
    return {}, {}


def run_export(c, **kw):
    from simplex_gp_amd import _native as nv
    names = ("KEYS", "ENTRY_VERTEX", "ENTRY_WEIGHT", "NEIGHBORS", "ROW_PTR", "CSR_POINT", "CSR_WEIGHT", "POINT_PERM")
    return {n: c.lat.export(getattr(nv, "ARRAY_" + n)).copy() for n in names}, {}


def run_row_order(c, **kw):
    """set_lattice_row_order on and off again: the op that follows turns it on for itself (Call.lattice_rows)."""
    c.lat.set_lattice_row_order(True)
    c.lat.set_lattice_row_order(False)
    return {}, {}


def judge_export(ref, res, **kw):
    """The structure against the CPU oracle's: as many vertices, the same set of keys (the bits are the twin's business)."""
    keys = np.asarray(res["KEYS"])
    same = keys.shape == ref.q64.xkeys.shape and {r.tobytes() for r in keys} == {r.tobytes() for r in ref.q64.xkeys}
    return [("keys exact", 0.0 if same else float("inf"))]


def _third(n):
    return n // 3, n // 2


# G1 single column fp32
op("apply_vd1", "G1", ["apply"], run_forward, judge_forward, tag="a1", vd=1)
op("stages_vd1", "G1", ["splat", "blur", "slice"], run_forward, judge_forward, tag="s1", vd=1, mode="stages")
# G2 multi column fp32
for _vd in (4, 11, 72):
    op(f"apply_vd{_vd}", "G2", ["apply"], run_forward, judge_forward, tag=f"a{_vd}", vd=_vd)
op("stages_vd11", "G2", ["splat", "blur", "slice"], run_forward, judge_forward, tag="s11", vd=11, mode="stages")
# G3 affine
op("affine_vd11", "G3", ["apply_affine"], run_forward, judge_affine, tag="af", vd=11, mode="affine")
op("affine_dot_vd11", "G3", ["apply_affine"], run_forward, judge_affine, tag="afd", vd=11, mode="dot", dot=True)
op("affine_partial_vd11", "G3", ["apply_affine"], run_forward, judge_affine, tag="afp", vd=11, mode="partial", dot=True)
# G4 the fused backward
op("backward_f32", "G4", ["apply_backward"], run_backward32, judge_backward32)
# G5 rows fp32
for _r in ("head", "tail", "overlap", "full"):
    for _vd in (1, 11):
        op(f"rows_{_r}_vd{_vd}", "G5", ["apply_rows"], run_rows, judge_rows32, tag=f"r{_r}{_vd}", rname=_r, vd=_vd)
op("rows_staged_vd11", "G5", ["splat_rows", "blur", "slice_rows"], run_rows, judge_rows32, tag="rs11", rname="overlap", vd=11,
   staged=True)
op("rows_recycle_vd3", "G5", ["apply_rows"], run_rows_cycle, judge_rows_cycle, tag="rc", vd=3)
op("backward_rows_f32", "G5", ["apply_backward_rows_f32"], run_backward_rows, judge_backward_rows, f64=False)
# G6 transposed / symmetrised fp32
op("apply_t_f32", "G6", ["apply_t_f32"], run_sym, judge_sym32, tag="t32", vd=11, which="t")
op("apply_sym_f32", "G6", ["apply_sym_f32"], run_sym, judge_sym32, tag="s32", vd=11, which="s")
op("affine_sym_f32", "G6", ["apply_affine_sym_f32"], run_sym, judge_sym32, tag="as32", vd=11, which="s", mode="affine", dot=True)
op("blur_sym_f32", "G6", ["splat", "blur_sym_f32", "slice"], run_sym, judge_sym32, tag="bs32", vd=11, which="s", mode="stages")
op("blur_t_f32", "G6", ["splat", "blur_t_f32", "slice"], run_sym, judge_sym32, tag="bt32", vd=3, which="t", mode="stages")
# G7 float64
for _vd in (1, 3, 12):
    op(f"apply64_vd{_vd}", "G7", ["apply"], run_apply64, judge_apply64, tag=f"d{_vd}", vd=_vd)
op("affine64_vd3", "G7", ["apply_affine"], run_apply64, judge_affine64, tag="daf", vd=3, mode="affine")
op("affine64_dot_vd3", "G7", ["apply_affine"], run_apply64, judge_affine64, tag="dafd", vd=3, mode="dot", dot=True)
# G8 rows float64
op("rows64_overlap_vd3", "G8", ["apply_rows"], run_rows, judge_rows64, tag="dr3", rname="overlap", vd=3, f64=True)
op("rows64_head_vd1", "G8", ["apply_rows"], run_rows, judge_rows64, tag="dr1", rname="head", vd=1, f64=True)
op("rows64_staged_vd3", "G8", ["splat_rows", "blur", "slice_rows"], run_rows, judge_rows64, tag="drs", rname="tail", vd=3,
   f64=True, staged=True)
op("rows64_recycle_vd2", "G8", ["apply_rows"], run_rows_cycle, judge_rows_cycle, tag="drc", vd=2, f64=True)
op("backward_rows_f64", "G8", ["apply_backward_rows"], run_backward_rows, judge_backward_rows, f64=True)
# G9 the float64 backward
op("backward_f64", "G9", ["apply_backward"], run_backward64, judge_backward64)
# G10 transposed / symmetrised float64
op("apply_t_f64", "G10", ["apply_t"], run_sym, judge_sym64, tag="t64", vd=3, which="t", f64=True)
op("apply_sym_f64", "G10", ["apply_sym"], run_sym, judge_sym64, tag="s64", vd=3, which="s", f64=True)
op("affine_sym_f64", "G10", ["apply_affine"], run_sym, judge_sym64, tag="as64", vd=3, which="s", f64=True, mode="affine", dot=True)
op("blur_t_f64", "G10", ["splat", "blur_t", "slice"], run_sym, judge_sym64, tag="bt64", vd=3, which="t", f64=True, mode="stages")
op("blur_sym_f64", "G10", ["splat", "blur_sym", "slice"], run_sym, judge_sym64, tag="bs64", vd=2, which="s", f64=True,
   mode="stages")
# G11 the diagonal
op("diag_f32", "G11", ["diag"], run_diag, judge_diag, f64=False)
op("diag_f64", "G11", ["diag"], run_diag, judge_diag, f64=True)
op("diag_f32_range", "G11", ["diag"], run_diag, judge_diag, f64=False, rows=_third)
op("diag_f64_lattice_rows", "G11", ["diag", "shard_perm"], run_diag, judge_diag, f64=True, lattice_rows=True)
# G12 queries
op("query_f32", "G12", ["locate", "splat", "blur", "slice_at"], run_query, judge_query, f64=False, vd=3)
op("query_f64", "G12", ["locate", "splat", "blur", "slice_at"], run_query, judge_query, f64=True, vd=3)
# G13 one-hot columns
op("splat_onehot", "G13", ["splat_onehot", "blur", "slice", "shard_perm"], run_onehot, judge_onehot, tag="oh", vd=4, nb=3,
   mode="splat")
op("filter_onehot_sparse", "G13", ["filter_onehot", "shard_perm"], run_onehot, judge_onehot, tag="ohs", vd=8, nb=8, mode="sparse")
op("filter_onehot_dense", "G13", ["filter_onehot", "shard_perm"], run_onehot, judge_onehot, tag="ohd", vd=4, nb=3, mode="dense")
# G14 housekeeping that must disturb nothing
op("prepare_vd1", "G14", ["prepare"], run_prepare, judge_nothing, vd=1)
op("prepare_vd11", "G14", ["prepare"], run_prepare, judge_nothing, vd=11)
op("export", "G14", ["export"], run_export, judge_export)
op("row_order", "G14", ["set_lattice_row_order", "to_lattice_order", "from_lattice_order", "shard_perm"], run_row_order,
   judge_nothing)

# blurred / apply_at are splat + blur and slice_at of them: the query ops make the same three calls on guarded buffers
COMPOSED_METHODS = {"blurred": ("splat", "blur"), "apply_at": ("blurred", "slice_at")}
# ops whose buffers may sit one element off a 16-byte boundary (their own modules run them so)
OFFSET_OK = ("apply_vd", "apply64_vd", "rows_", "rows64_", "apply_t_", "apply_sym_", "backward_f64", "backward_rows_")


def offset_of(opname):
    return seed_of("offset", opname) & 1 if opname.startswith(OFFSET_OK) else 0


def do_build(lat, rf, build, dev):
    """Build `build` of the chain on `lat`.  dev: {build: positions on the device}.  Returns filter_once's result or None."""
    import torch
    ref = rf[build]
    if build == "once":
        src = torch.from_numpy(ref.rhs("once", ref.n, 3)).cuda()
        return _np(lat.filter_once(src, dev[build], ref.taps))
    lat.build(dev[build], ref.taps, reuse_order=(build == "warm"))
    return None


def replay(rf, build, dev):
    """A fresh Lattice that made only the builds since and including the last cold one."""
    import simplex_gp_amd as plx
    twin = plx.Lattice()
    once = None
    for b in (("cold", "warm") if build == "warm" else (build,)):
        once = do_build(twin, rf, b, dev)
    return twin, once


class Runner:
    """One scenario on one Lattice object: run(seq) plays a sequence and checks every step."""

    def __init__(self, scn):
        import torch
        import simplex_gp_amd as plx
        from tests.gpubuf import Buf
        self.scn, self.rf = scn, refs(scn)
        self.lat = plx.Lattice()
        self.xbuf = {b: Buf(torch.from_numpy(r.x), dtype=torch.float32) for b, r in self.rf.items() if b != "again"}
        self.xbuf["again"] = self.xbuf["cold"]
        self.dev = {b: buf.view.view(self.rf[b].n, self.rf[b].d) for b, buf in self.xbuf.items()}
        self.keys = {}
        self.worst, self.steps_run, self.kernels_seen, self.block_rows = {}, 0, {}, 0

    def device_keys(self, build):
        """The vertex keys in the device's numbering, from a scout that replayed the builds (no call on the object)."""
        from simplex_gp_amd import _native as nv
        if build not in self.keys:
            scout, _ = replay(self.rf, build, self.dev)
            self.keys[build] = scout.export(nv.ARRAY_KEYS).copy()
            scout.close()
        return self.keys[build]

    def note(self, opname, items):
        for _, ratio in items:
            self.worst[opname] = max(self.worst.get(opname, 0.0), ratio)

    def run_op(self, lat, build, opname, lattice_rows):
        o = OPS[opname]
        c = Call(lat, self.rf[build], offset_of(opname), lattice_rows)
        kw = dict(o.kw)
        c.single_use = build == "once"
        if o.group == "G12":
            kw["keys"] = self.device_keys("cold" if build == "again" else build)
        res, kern = o.run(c, **kw)
        c.check()
        return res, kern

    def run(self, seq, label=""):
        from tests.test_forward_fp64 import ENTRY, REL
        for chain in seq:
            first_segment = {}
            for build, seg in zip(BUILDS, chain):
                ref = self.rf[build]
                once = do_build(self.lat, self.rf, build, self.dev)
                assert self.lat.m == ref.l64.m, (label, build, "vertices", self.lat.m, ref.l64.m)
                if once is not None:
                    twin, twin_once = replay(self.rf, build, self.dev)
                    twin.close()
                    v = ref.rhs("once", ref.n, 3)
                    want, T = ref.cached(("fwd", "once", 3), lambda: fwd_reference(ref, v))
                    items = item_entry("out", once, want, T, ENTRY, REL)
                    assert all(r <= 1.0 for _, r in items), (label, "filter_once", items)
                    assert values_equal(once, twin_once), (label, "filter_once differs from a fresh lattice's")
                    self.note("filter_once", items)
                earlier, rows_on = None, False
                for i, opname in enumerate(seg):
                    where = f"{label} {build}[{i}]"
                    res, kern = self.run_op(self.lat, build, opname, rows_on)
                    twin, _ = replay(self.rf, build, self.dev)
                    try:
                        tres, tkern = self.run_op(twin, build, opname, rows_on)
                    finally:
                        twin.close()
                    first = first_segment.get((i, opname)) if build == "again" else None
                    assert build != "again" or first is not None, (where, "the last segment repeats the first")
                    items = check_step(opname, ref, res, tres, kern, tkern, first=first, earlier=earlier, label=where)
                    if build == "cold":
                        first_segment[(i, opname)] = res
                    self.note(opname, items)
                    self.kernels_seen[(build, opname)] = kern
                    if opname == "apply_vd1" and build in ("cold", "again"):
                        self.block_rows = self.lat.block_rows
                    self.steps_run += 1
                    rows_on = opname == "row_order"
                    earlier = opname
        for buf in self.xbuf.values():
            assert buf.unchanged() and buf.guards_intact(), (label, "the positions were written")

    def close(self):
        self.lat.close()
