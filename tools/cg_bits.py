"""Dump the bits of the CG vector steps for the library PLX_LIBRARY names (default: the tree's libplx.so), to compare two
builds of the library byte for byte:

    PLX_LIBRARY=/path/to/libplx.so python tools/cg_bits.py > dump.txt        (one process per library, then cmp)

The nine entry points of plx_cg_kernels.h: plx_coldot, plx_cg_update, plx_cg_step_update, plx_cg_step_direction and
plx_pcg_step_direction over n in (0, 1, 2, 1023, 1025, 4100) x vd in (1, 3, 11, 12, 16, 255, 256); plx_coldot_f64,
plx_cg_step_update_f64, plx_cg_step_direction_f64 and plx_pcg_step_direction_f64 over NS x VDS of tests/test_cg_f64_gpu.py.
Every shape runs with its first matrix (a, X, P) aligned and one element past alignment.  Column c of the scalars is
inactive at c % 4 == 1, has rs = 0 at c % 4 == 2 and pAp <= 0 at c % 4 == 3; the activity test puts the others on either
side of tol.  Then four khat_solve runs on cloud("gauss1", 2000, 3, seed=1) (RBF order 1, noise 1.0, check_every = 4,
tridiagonals on): fp32 with a rank-100 preconditioner on 12 columns with FUSED_CG_STEPS "auto" and False, float64 plain and
float64 with rank 100 on 3 columns.  One line per output buffer: the call, the shape, the offset, the buffer, its byte
count, the SHA-256 of its bytes and the count of non-finite values.  Needs a GPU.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplex_gp_amd as plx  # noqa: E402
from simplex_gp_amd import _native as nv  # noqa: E402
from simplex_gp_amd import solvers  # noqa: E402
from tests import test_cg_f64_gpu as t64  # noqa: E402
from tests.lattice64 import cloud  # noqa: E402

NS32, VDS32 = (0, 1, 2, 1023, 1025, 4100), (1, 3, 11, 12, 16, 255, 256)
TOL = 1e-3


def emit(call, shape, off, outs):
    torch.cuda.synchronize()
    for what, t in outs:
        raw = t.contiguous().cpu().numpy().tobytes()
        bad = int((~torch.isfinite(t)).sum())
        print(f"{call} {shape} off={off} {what} {len(raw)} {hashlib.sha256(raw).hexdigest()} nonfinite={bad}", flush=True)


def placed(host, off):
    """a device copy of `host`, `off` elements past the (256-byte aligned) start of its allocation"""
    raw = torch.empty(off + host.numel() + 1, dtype=host.dtype, device="cuda")
    view = raw[off: off + host.numel()]
    view.copy_(host.reshape(-1))
    view.raw = raw          # (an empty view has no address of its own: n = 0 still passes a valid pointer)
    return view


def p(t):
    raw = getattr(t, "raw", None)
    return ctypes.c_void_p(t.data_ptr() if raw is None else raw.data_ptr() + t.storage_offset() * t.element_size())


def vector_calls(f64, n, vd, off):
    lib, dtype, sfx = nv.lib(), (torch.float64 if f64 else torch.float32), ("_f64" if f64 else "")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(1000 * n + vd)
    mats = [torch.randn(n, vd, generator=g, dtype=torch.float64).to(dtype) for _ in range(4)]
    col = torch.arange(vd)
    rs, pap, rr = (torch.rand(vd, generator=g, dtype=torch.float64).add(0.5).mul(max(n, 1)) for _ in range(3))
    rs_new = torch.rand(vd, generator=g, dtype=torch.float64).add(0.5).mul(max(n, 1))
    active = torch.where(col % 4 == 1, 0.0, 1.0)
    rs = torch.where(col % 4 == 2, 0.0, rs)
    pap = torch.where(col % 4 == 3, -0.25, pap)
    side = torch.where(col % 2 == 0, 0.5, 2.0)
    dev = lambda t: t.to(dtype).cuda()      # noqa: E731
    RS, PAP, RSN, RR, ACT, ALPHA = (dev(t) for t in (rs, pap, rs_new, rr, active, torch.randn(vd, generator=g, dtype=torch.float64)))
    work = torch.empty(int(lib.plx_coldot_work_doubles(vd) if f64 else lib.plx_coldot_work_floats(vd)), dtype=dtype, device="cuda")
    out = lambda: torch.zeros(vd, dtype=dtype, device="cuda")      # noqa: E731
    shape = f"n={n} vd={vd}"
    # column dots
    a, b, dot = placed(mats[0], off), placed(mats[1], 0), out()
    nv.check(getattr(lib, "plx_coldot" + sfx)(p(a), p(b), n, vd, p(dot), p(work), st), "plx_coldot" + sfx)
    emit("plx_coldot" + sfx, shape, off, (("out", dot),))
    # the updates
    if not f64:
        X, R, P, AP, rsn = placed(mats[0], off), placed(mats[1], 0), placed(mats[2], 0), placed(mats[3], 0), out()
        nv.check(lib.plx_cg_update(p(X), p(R), p(P), p(AP), p(ALPHA), n, vd, p(rsn), p(work), st), "plx_cg_update")
        emit("plx_cg_update", shape, off, (("X", X), ("R", R), ("rs_new", rsn)))
    X, R, P, AP, rsn, alpha = placed(mats[0], off), placed(mats[1], 0), placed(mats[2], 0), placed(mats[3], 0), out(), out()
    name = "plx_cg_step_update" + sfx
    nv.check(getattr(lib, name)(p(X), p(R), p(P), p(AP), p(RS), p(PAP), p(ACT), n, vd, p(rsn), p(alpha), p(work), st), name)
    emit(name, shape, off, (("X", X), ("R", R), ("rs_new", rsn), ("alpha", alpha)))
    # the direction steps: the activity test on either side of tol
    for pcg in (False, True):
        BN = dev((rr if pcg else rs_new).sqrt() / TOL * side)
        P, S, beta, act = placed(mats[2], off), placed(mats[1], 0), out(), out()
        name = ("plx_pcg_step_direction" if pcg else "plx_cg_step_direction") + sfx
        args = (p(P), p(S), p(RSN), p(RS)) + ((p(RR),) if pcg else ()) + (p(ACT), p(BN), TOL, n, vd, p(beta), p(act), st)
        nv.check(getattr(lib, name)(*args), name)
        emit(name, shape, off, (("P", P), ("beta", beta), ("active_out", act)))


def solves():
    x64 = torch.from_numpy(np.ascontiguousarray(cloud("gauss1", 2000, 3, seed=1))).double()
    g = torch.Generator().manual_seed(5)
    rhs64 = torch.randn(2000, 12, generator=g, dtype=torch.float64)
    default = solvers.FUSED_CG_STEPS
    runs = (("fp32 rank 100 fused auto", False, 100, 12, 1e-5, "auto"), ("fp32 rank 100 fused off", False, 100, 12, 1e-5, False),
            ("float64 plain", True, 0, 3, 1e-11, default), ("float64 rank 100", True, 100, 3, 1e-11, default))
    try:
        for name, f64, rank, cols, tol, fused in runs:
            solvers.FUSED_CG_STEPS = fused
            dtype = torch.float64 if f64 else torch.float32
            model = solvers.LatticeGP(plx.RBFLattice(order=1, ard_num_dims=3)).to(dtype).cuda()
            x, rhs = x64.to(dtype).cuda(), rhs64[:, :cols].to(dtype).contiguous().cuda()
            with torch.no_grad():
                model.raw_noise.fill_(float(np.log(np.expm1(1.0 - model.min_noise))))          # noise 1.0
                K = model.kernel(x, x)
                pre = model.preconditioner(x, rank, K=K) if rank else None
                sol, info = model.khat_solve(x, rhs, K=K, max_iter=500, tol=tol, check_every=4, want_tridiag=True, precond=pre)
            its = torch.tensor([int(info["iterations"])])
            emit("khat_solve", name.replace(" ", "_"), 0, (("X", sol), ("residual", info["residual"]), ("tridiag", info["tridiag"]),
                                                          ("iterations", its)))
            plx.lattice_cache().clear()
    finally:
        solvers.FUSED_CG_STEPS = default


def main():
    if not torch.cuda.is_available():
        raise SystemExit("cg_bits.py needs a GPU")
    for n in NS32:
        for vd in VDS32:
            for off in (0, 1):
                vector_calls(False, n, vd, off)
    for n in t64.NS:
        for vd in t64.VDS:
            for off in (0, 1):
                vector_calls(True, n, vd, off)
    solves()


if __name__ == "__main__":
    main()
