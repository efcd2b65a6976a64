"""float64 references, error measures and the kernel-family table for the native solver kernels (plx_linalg.hip,
plx_cg_kernels.h, plx_pcg.hip, plx_lanczos_kernels.h).  Plain numpy on the CPU: tests/test_solver64.py checks these helpers without a GPU,
tests/test_solver_fp64.py holds the kernels against them.

The measure follows lattice64.terms64 / entry_ratio: every output entry is compared with its float64 value in units of
the sum of the absolute values of the terms that entry adds up; where that sum is 0 the entry must be exactly 0.
Every reference takes the SAME fp32 values the kernel received (for an fp16 factor: the rounded values) and evaluates
the same expression in float64."""
import os
import re

import numpy as np

TINY = 1e-30            # the max(x, tiny) guard of the fp32 CG coefficients (plx_cg_kernels.h: Cg<float>::guard)
EPS32 = 2.0 ** -24      # half an ulp of fp32, relative

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("plx_linalg.hip", "plx_cg_kernels.h", "plx_pcg.hip", "plx_lanczos_kernels.h")
NOT_OURS = ("backward_stack_kernel", "backward_contract_kernel")      # DESIGN section 10 owns them


def f64(a):
    return np.asarray(a, np.float64)


FLT_MIN = 2.0 ** -126   # the smallest normal fp32: a result below it may be flushed to zero


def entry_ratio(got, want, T, floor=0.0):
    """max over the entries of |got - want| / T; an entry whose terms sum T is 0 must be exactly 0 (else inf), and
    no entry may be NaN or inf.  floor: an absolute error every entry is allowed before the ratio counts (FLT_MIN where
    the data reaches below the fp32 normal range: the GPU flushes subnormal results to zero)."""
    got, want, T = np.broadcast_arrays(f64(got), f64(want), f64(T))
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.maximum(np.abs(got - want) - floor, 0.0)
    zero = T == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float((err[~zero] / T[~zero]).max()) if np.any(~zero) else 0.0


def rel_ratio(got, want):
    """max |got - want| / |want| (a coefficient against its fp64 value); want = 0 demands got = 0."""
    return entry_ratio(got, want, np.abs(f64(want)))


# ---- references ------------------------------------------------------------------------------------------------------
def coldot64(a, b):
    """(sum_r a b, sum_r |a b|) per column of two [n][vd] matrices."""
    p = f64(a) * f64(b)
    return p.sum(0), np.abs(p).sum(0)


def colsum64(part):
    """(sum, sum of |.|) over the rows of a [rows][vd] matrix of partial sums."""
    p = f64(part)
    return p.sum(0), np.abs(p).sum(0)


def axpy64(y, a, x):
    """(y + a x, |y| + |a x|) with a per column: X += alpha P, R -= alpha AP (a = -alpha), P = R + beta P."""
    y, a, x = f64(y), f64(a), f64(x)
    return y + a * x, np.abs(y) + np.abs(a * x)


def alpha64(rs, pap, active):
    """alpha = active ? rs / max(pAp, tiny) : 0 (include/plx.h) from the fp32 scalars."""
    with np.errstate(over="ignore"):
        return np.where(f64(active) > 0, f64(rs) / np.maximum(f64(pap), TINY), 0.0)


beta64 = alpha64      # beta = active ? rs_new / max(rs, tiny) : 0: the same expression


def active64(active, rr, b_norm, tol, margin=1e-3):
    """(flag, decided): flag = active and sqrt(rr) / b_norm > tol as fp64 evaluates it; decided[c] is False where the
    fp64 value lies within `margin` (relative) of tol, i.e. where rounding could decide the flag."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.sqrt(f64(rr)) / f64(b_norm)
    on = f64(active) > 0
    flag = (on & (q > tol)).astype(np.float32)          # NaN > tol is False, inf > tol is True: as the kernel's comparison
    decided = ~on | ~np.isfinite(q) | (np.abs(q - tol) >= margin * abs(tol))
    return flag, decided


def project64(L, R, cinv):
    """T = Cinv (L^T R) and its terms |Cinv| (|L|^T |R|); L is [kp][n] (the factor's rows, tail cut), R [n][t]."""
    L, R, cinv = f64(L), f64(R), f64(cinv)
    return cinv @ (L @ R), np.abs(cinv) @ (np.abs(L) @ np.abs(R))


def apply64(L, k, R, T, scale):
    """Z = (s0 R - L[:k]^T T[:k]) s1 and its terms (|s0 R| + |L|^T |T|) |s1| per entry; T is the device's [kp][16]."""
    L, R, T = f64(L)[:k], f64(R), f64(T)[:k, :np.shape(R)[1]]
    s0, s1 = float(scale[0]), float(scale[1])
    return (s0 * R - L.T @ T) * s1, (np.abs(s0 * R) + np.abs(L).T @ np.abs(T)) * abs(s1)


def lanczos_step64(Q, w, i):
    """One plx_lanczos_step in float64.  Q: [i + 1][n] basis rows, w: [n].  The kernel's recurrence: the components along
    rows i - 1 and i are removed first (alpha's first part is the coefficient of row i), then one classical Gram-Schmidt
    pass against rows 0..i (alpha's second part), beta = the norm of what is left, next vector = w / max(beta, 1e-30).
    Returns a dict: w (un-normalised), alpha, beta, q, and the terms of each: Tw per entry (|w| + sum_j |c_j| |q_j|, c_j
    the total coefficient removed along row j), Talpha (sum of |Q_i w| over both passes), Tbeta2 (= beta^2: squares)."""
    Q, w = f64(Q)[: i + 1], f64(w)
    rows, first = i + 1, max(0, i - 1)
    c0 = np.zeros(rows)
    c0[first:] = Q[first:] @ w
    t0 = np.abs(Q[i]) @ np.abs(w)
    w1 = w - c0[first:] @ Q[first:]
    c2 = Q @ w1
    t2 = np.abs(Q[i]) @ np.abs(w1)
    w2 = w1 - c2 @ Q
    beta = float(np.sqrt(w2 @ w2))
    return dict(w=w2, alpha=float(c0[i] + c2[i]), beta=beta, q=w2 / max(beta, 1e-30),
                Tw=np.abs(w) + (np.abs(c0) + np.abs(c2)) @ np.abs(Q), Talpha=float(t0 + t2), Tbeta2=float(w2 @ w2))


def pchol64(A, diag, L_done, steps, tol_abs, rank=None, allowed=None):
    """Sequential pivoted Cholesky in float64, continued from a given state: A [n][n] (symmetric), diag [n] the residual
    diagonal, L_done [m][n] the finished columns (as rows).  Runs up to `steps` steps; with `allowed` (a set of rows) it
    stops before the first step whose argmax is not in it (a batch only holds its candidates' kernel rows).
    Ties go to the LOWER rank (rank None: the lower index).  A pivot <= tol_abs gives a zero column.
    Returns (pivots, columns [a][n], terms [a][n], diag, gaps): terms = (|row| + sum_j |L_ij| |L_pj|) / sqrt(pivot), gaps[s] =
    relative distance between the two largest diagonal entries when step s chose."""
    A, d = f64(A), f64(diag).copy()
    n = d.size
    rank = np.arange(n) if rank is None else np.asarray(rank, np.int64)
    Ls = [f64(r) for r in L_done]
    pivots, cols, terms, gaps = [], [], [], []
    for _ in range(steps):
        top = d.max()
        p = int(min(np.flatnonzero(d == top), key=lambda i: rank[i]))
        if allowed is not None and p not in allowed:
            break
        second = np.partition(d, -2)[-2] if n > 1 else 0.0
        gaps.append((top - second) / top if top > 0 else 0.0)
        Lm = np.array(Ls) if Ls else np.zeros((0, n))
        v = A[:, p] - Lm.T @ Lm[:, p]
        tv = np.abs(A[:, p]) + np.abs(Lm).T @ np.abs(Lm[:, p])
        root = np.sqrt(max(top, 1e-30))
        col = v / root if top > tol_abs else np.zeros(n)
        d = np.maximum(d - col * col, 0.0)
        d[p] = 0.0
        Ls.append(col)
        pivots.append(p)
        cols.append(col)
        terms.append(tv / root if top > tol_abs else np.zeros(n))
    return pivots, np.array(cols).reshape(len(cols), n), np.array(terms).reshape(len(terms), n), d, gaps


def pchol_columns_given(A, diag, L_done, got_cols, pivots, tol_abs):
    """The columns of a batch, each from the fp32 columns BEFORE it as the kernel stored them (got_cols [a][n]) -- the
    inputs its own step read -- instead of from the float64 chain: column j = (A[:, p_j] - sum_q L_iq L_pq) / sqrt(d_p),
    d_p = diag[p] - sum over the batch's earlier columns of L_pq^2.  An error of an earlier column is judged in that column,
    not again (amplified by cancellation) in every later one.  Returns (columns, terms) like pchol64."""
    A, d0 = f64(A), f64(diag)
    n = d0.size
    prev = [f64(r) for r in L_done]
    cols, terms = [], []
    for j, p in enumerate(pivots):
        Lm = np.array(prev + [f64(c) for c in got_cols[:j]]).reshape(len(prev) + j, n)
        dp = max(d0[p] - sum(float(f64(c)[p]) ** 2 for c in got_cols[:j]), 0.0)
        root = np.sqrt(max(dp, 1e-30))
        v = A[:, p] - Lm.T @ Lm[:, p]
        tv = np.abs(A[:, p]) + np.abs(Lm).T @ np.abs(Lm[:, p])
        ok = dp > tol_abs
        cols.append(v / root if ok else np.zeros(n))
        terms.append(tv / root if ok else np.zeros(n))
    return np.array(cols).reshape(len(cols), n), np.array(terms).reshape(len(terms), n)


def top_candidates(diag, nb, rank=None):
    """What plx_pchol_select must return: the nb largest entries, larger first, ties by lower rank."""
    d = f64(diag)
    rank = np.arange(d.size) if rank is None else np.asarray(rank, np.int64)
    return [int(i) for i in sorted(range(d.size), key=lambda i: (-d[i], rank[i]))[:nb]]


# ---- which kernels a call runs: the dispatch rules of the four sources, restated ---------------------------------------
K_BLOCK = 256
DOT_BLOCKS = 1024             # coldot / cg_update / cg_step_update: workgroups = rows of partial sums
FINAL_BLOCK = 1024
FUSED_BLOCKS = 256            # rows of |R|^2 partial sums cg_step_update_fused leaves
LZ_MAX_ROWS, LZ_MAX_GROUPS = 256, 256
LZ_SPANS = (256, 1024, 4096, 8192)
GRAM_BLOCKS = 512             # default workgroups of the gram kernel = partial sums per entry
HALF = {False: "f32", True: "f16"}


def final_family(nblocks):
    """coldot_final_kernel: its four-way unrolled loop only runs with more than 3 * 1024 rows of partial sums."""
    return "coldot_final_kernel/unrolled" if nblocks > 3 * FINAL_BLOCK else "coldot_final_kernel/tail"


def coldot_families(kernel):
    return [kernel, final_family(DOT_BLOCKS)]


def direction_family(prefix, n, vd, aligned):
    """plx_cg_step_direction (prefix 'cg') / plx_pcg_step_direction ('pcg'), one pair of kernels with src = R / Z: four
    elements per thread when n vd is a positive multiple of 4 and both streamed matrices are 16-byte aligned, else the
    scalar kernel."""
    total = n * vd
    return f"step_direction_vec_kernel/{prefix}" if total > 0 and total % 4 == 0 and aligned else f"step_direction_kernel/{prefix}"


def fused_family(kernel, vd):
    assert vd in (4, 8, 12, 16)
    return f"{kernel}<{vd // 4}>"


def gram_families(kp, half):
    """one launch per 128 rows of L^T, JT = row tiles of 16 in it"""
    return [f"pcg_gram_kernel<{min(8, (kp - j0) // 16)},{HALF[half]}>" for j0 in range(0, kp, 128)]


def project_families(kp, half):
    return gram_families(kp, half) + ["pcg_project_kernel"]


def rz_rows(n, half):
    return -(-n // (K_BLOCK * (2 if half else 1)))


def apply_families(n, t, half, with_rz):
    fam = [f"pcg_apply_kernel<{t},rows,{HALF[half]}>"]
    if with_rz:
        fam.append(final_family(rz_rows(n, half)))
    return fam


def pchol_batch_families(m_done, t, nb, exact_steps):
    fam = ["pchol_top_partial_kernel", "pchol_top_final_kernel", f"pcg_apply_kernel<{t},transposed,f32>", "pchol_plan_kernel",
           "pchol_multi_step_kernel"]
    if m_done > 0:
        fam.append("pchol_gather_kernel")
    if exact_steps and nb > 1:
        fam.append("pchol_step_kernel")
    return fam


def lanczos_span(n):
    """rows per workgroup, or None beyond the 8192 x 256 rows a step serves"""
    for span in LZ_SPANS:
        if n <= span * LZ_MAX_GROUPS:
            return span
    return None


def lanczos_families(n):
    span = lanczos_span(n)
    return [f"lanczos_{k}_kernel<{span}>" for k in ("project", "subtract_project", "subtract_norm", "scale")]


def _families():
    fam = {}

    def add(name, reached_by):
        fam[name] = reached_by
    add("coldot_partial_kernel", "test_coldot")
    add("coldot_final_kernel/tail", "test_coldot, test_cg_updates, test_pcg_apply (d_rz given, up to 3072 partial rows)")
    add("coldot_final_kernel/unrolled", "test_pcg_apply_large (n = 1,100,000, fp32 factor: 4297 partial rows)")
    add("cg_update_kernel/alpha", "test_cg_updates (plx_cg_update: alpha given)")
    add("cg_update_kernel/step", "test_cg_updates (plx_cg_step_update: alpha formed on the device)")
    add("cg_direction_kernel", "test_cg_updates")
    add("step_direction_kernel/cg", "test_step_direction (n vd odd, or P 4 bytes past a 16-byte boundary)")
    add("step_direction_vec_kernel/cg", "test_step_direction (n vd a multiple of 4, aligned)")
    add("step_direction_kernel/pcg", "test_step_direction")
    add("step_direction_vec_kernel/pcg", "test_step_direction")
    for nch in (1, 2, 3, 4):
        add(f"cg_step_update_fused_kernel<{nch}>", f"test_fused_steps (vd = {4 * nch})")
        add(f"cg_step_direction_fused_kernel<{nch}>", f"test_fused_steps (vd = {4 * nch})")
        add(f"pcg_step_direction_fused_kernel<{nch}>", f"test_fused_steps (vd = {4 * nch})")
    for half in (False, True):
        for jt in range(1, 9):
            add(f"pcg_gram_kernel<{jt},{HALF[half]}>", f"test_pcg_project (kp = {16 * jt}, or kp = 128 q + {16 * jt % 128})")
        for t in range(1, 17):
            add(f"pcg_apply_kernel<{t},rows,{HALF[half]}>", f"test_pcg_apply (t = {t})")
    for t in range(1, 17):
        add(f"pcg_apply_kernel<{t},transposed,f32>", f"test_pchol_batch / test_pchol_panel_widths (t = {t})")
    add("pcg_project_kernel", "test_pcg_project")
    add("pcg_to_half_kernel", "test_factor_to_half, test_pcg_project / test_pcg_apply (fp16 factor)")
    for k in ("top_partial", "top_final", "onehot", "gather", "plan", "multi_step", "step"):
        add(f"pchol_{k}_kernel", "test_pchol_batch" + (" (exact_steps, a strongly coupled matrix)" if k == "step" else ""))
    for span in LZ_SPANS:
        for k in ("project", "subtract_project", "subtract_norm", "scale"):
            add(f"lanczos_{k}_kernel<{span}>", f"test_lanczos_step (rows per workgroup {span})")
    return fam


FAMILIES = _families()
# families no argument of the C ABI selects: name -> reason (at most 3; DESIGN section 12 justifies each)
UNREACHABLE = {}


def family_kernel(name):
    return re.split(r"[</]", name)[0]


def family_values(name):
    """the integer template values a family name carries"""
    m = re.search(r"<([^>]*)>", name)
    return [int(x) for x in re.findall(r"\d+", m.group(1).split(",")[0])] if m else []


def _source(src, root):
    return re.sub(r"//[^\n]*", "", open(os.path.join(root, "simplex_gp_amd", "csrc", src)).read())


def ladder_spans(root=ROOT, src="plx_lanczos_kernels.h"):
    """{"float": [...], "double": [...]}: the spans of each LzScalar<T>::kLadder, the only values the templated dispatch
    (lz_dispatch<T, K>: lanczos_launch<T, LzScalar<T>::kLadder[K].span>) instantiates for T."""
    text = _source(src, root)
    spans = {}
    for m in re.finditer(r"struct\s+LzScalar<(\w+)>\s*\{(.*?)\n\};", text, re.S):
        rungs = re.search(r"kLadder\[\]\s*=\s*\{(.*?)\};", m.group(2), re.S)
        spans[m.group(1)] = [int(v) for v in re.findall(r"\{\s*(\d+)\s*,", rungs.group(1))]
    return spans


def parse_sources(root=ROOT):
    """(kernels, pairs): every __global__ kernel name of the three sources, and every (kernel, value) pair their
    switch statements dispatch: `case N: kernel<N...>` / `default: kernel<N>`, `case N: launcher<N>(...)` for a host
    template that launches kernel<SPAN>s, and every PLX_*_CASE(N) invocation of a macro whose body names kernel<...>.
    A host template over <typename T, int SPAN> that launches kernel<T, SPAN>s and is called with a rung of the type's
    ladder (`launcher<T, SPAN>` with SPAN = LzScalar<T>::kLadder[K].span) dispatches the spans of the FLOAT ladder: the
    fp32 families keep their names, kernel<span>; ladder_spans has the double ladder."""
    kernels, pairs = set(), set()
    for src in SOURCES:
        text = _source(src, root)
        kernels.update(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\(", text))
        # host templates that launch kernels with their own template value: launcher -> kernels
        launchers, typed = {}, set()
        for m in re.finditer(r"template\s*<(typename T,\s*)?int (\w+)>\s*static\s+\w+\s+(\w+)\s*\(", text):
            body = text[m.end(): text.find("\n}\n", m.end())]
            launched = set(re.findall(r"(\w+_kernel)<%s%s>" % ("T, " if m.group(1) else "", m.group(2)), body))
            launchers[m.group(3)] = launched
            if m.group(1) and launched:
                typed.add(m.group(3))
        for m in re.finditer(r"(?:case\s+(\d+)|default)\s*:\s*(\w+)<(\d+)[,>]", text):
            value, callee = int(m.group(3)), m.group(2)
            assert m.group(1) is None or int(m.group(1)) == value or callee in launchers, m.group(0)
            for k in launchers.get(callee, {callee}):
                pairs.add((k, value))
        for launcher in typed:
            # the one call: from the ladder walk, with the rung's span
            calls = re.findall(r"\b%s<T, (\w+)>\(" % launcher, text)
            assert calls == ["SPAN"] and re.search(r"constexpr int SPAN = LzScalar<T>::kLadder\[K\]\.span;", text), (launcher, calls)
            pairs.update((k, span) for k in launchers[launcher] for span in ladder_spans(root, src)["float"])
        for m in re.finditer(r"#define\s+(PLX_\w*CASE)\((\w+)\)((?:[^\n]*\\\n)*[^\n]*)\n", text):
            macro, body = m.group(1), m.group(3)
            named = set(re.findall(r"(\w+_kernel)<", body))
            for v in re.findall(r"\b%s\((\d+)\)" % macro, text):
                pairs.update((k, int(v)) for k in named)
    return kernels, pairs
