#!/usr/bin/env python3
"""Randomised check of LatticeFilterGeneral's gradients on the HIP path (fused plx_apply_backward where the shape
allows, the three-call native form otherwise) against float64 (tests/lattice64.py: the same duplicate-free structure,
every sum in float64).  d = 1..32; RBF orders 1-3 and Matern-1.5 order 3 (forward and derivative taps differ there).

grad_x is a difference of products (py:122) that vanishes where points are isolated, so it is judged against the size of
those products T (lattice64.contract64): ||got - want|| <= 1e-5 ||T||, and rel-L2 <= 2e-5 only where ||want|| >= 0.1 ||T||.
grad_src and the output: rel-L2 <= 1e-5."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import simplex_gp_amd as plx
from tests.lattice64 import Lattice64, contract64, grad_x_ratios, rel_l2, stack64
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
TAU, REL_X, REL = 1e-5, 2e-5, 1e-5

kernels = [plx.DiscretizedKernelFN(plx.rbf, 1), plx.DiscretizedKernelFN(plx.rbf, 2), plx.DiscretizedKernelFN(plx.rbf, 3),
           plx.DiscretizedKernelFN(lambda d2: plx.Matern.apply(d2, 1.5), 3)]
worst = {"grad_x/T": (0.0, None), "grad_x rel": (0.0, None), "grad_src": (0.0, None), "out": (0.0, None)}
nfused = nvanish = 0
for c in range(cases):
    n = int(rng.choice([1, 5, 64, 300, 1025, 3000]))
    d = int(rng.integers(1, 33))
    L = int(rng.choice([1, 2, 3, 7, 8, 11, 16, 20, 28]))
    dk = kernels[int(rng.integers(0, len(kernels)))]
    scale = float(rng.choice([0.1, 0.3, 1.0, 3.0]))
    x0 = (rng.standard_normal((n, d)) * scale).astype(np.float32)
    v0 = rng.standard_normal((n, L)).astype(np.float32)
    w0 = rng.standard_normal((n, L)).astype(np.float32)
    only_x = bool(rng.integers(0, 2))
    x = torch.from_numpy(x0).cuda().requires_grad_(True)
    v = torch.from_numpy(v0).cuda().requires_grad_(not only_x)
    out = plx.LatticeFilterGeneral.apply(v, x, dk)
    (out * torch.from_numpy(w0).cuda()).sum().backward()
    plx.lattice_cache().clear()
    nfused += int(plx.Lattice.backward_fusable(L, d))
    lat64 = Lattice64(x0, dk.get_deriv_coeffs().numpy())
    gx64, gs64, T = contract64(w0, v0, x0, lat64.apply_staged(stack64(w0, v0, x0)))
    out64 = Lattice64(x0, dk.get_coeffs().numpy()).apply_staged(v0)
    terms, rel = grad_x_ratios(x.grad.cpu().numpy(), gx64, T)
    nvanish += int(rel is None)
    errs = {"grad_x/T": terms, "grad_x rel": rel, "out": rel_l2(out.detach().cpu().numpy(), out64),
            "grad_src": None if only_x else rel_l2(v.grad.cpu().numpy(), gs64)}
    bars = {"grad_x/T": TAU, "grad_x rel": REL_X, "out": REL, "grad_src": REL}
    for name, e in errs.items():
        if e is None:
            continue
        if e > worst[name][0]:
            worst[name] = (e, (n, d, L, scale, c))
        if not e <= bars[name]:
            print("FAIL", name, e, (n, d, L, scale, c), flush=True)
            sys.exit(1)
print(f"{cases} cases ({nfused} through the fused kernel, {nvanish} with a vanishing grad_x judged against its terms only):")
for name, (e, where) in worst.items():
    print(f"  worst {name}: {e:.2e} at (n, d, L, scale, case) = {where}")
