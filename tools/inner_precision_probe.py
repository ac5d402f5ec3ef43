#!/usr/bin/env python3
"""CPU probe behind the opt-in inner precision (include/nsx.h: NSX_INNER_FP32): does an inner GMRES on F, preconditioned with the
per-rank ILU(0) of F, take the same number of iterations when the VALUES of F and the off-diagonal entries of the factors are rounded
to float and back (the inverse pivots stay double)?  Matrices and factors come from the test oracle; the solver is SciPy's restarted
GMRES (restart 28), not deal.II's recurrences -- the counts say how the rounding moves a Krylov solve, not what libnsx will count.
A tool, not a test; needs no GPU.

    python tools/inner_precision_probe.py [--dim 3] [--level 2] [--ranks 24] [--ordering colour]
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--ranks", type=int, default=24)
    ap.add_argument("--ordering", default="colour")
    a = ap.parse_args()
    import oracle
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh = Mesh.cylinder(a.dim, a.level)
    if a.ranks > 1:
        mesh.partition(1, a.ranks)
    dofs, dt = DoFs(mesh, a.ordering), (2e-4 if a.dim == 3 else 1e-2)
    ora = oracle.Oracle(dofs, Tables(a.dim), 1e-3, dt)
    rng = np.random.default_rng(1234)
    ora.solution[:] = 0.3 * rng.standard_normal(dofs.n_dofs)
    ora.assemble(nsx.TEMAM)
    ora.apply_boundary_values(*cylinder_boundary_values(dofs, InletVelocity(a.dim, 2 if a.dim == 3 else 3), dt))
    ora.prec_initialize(nsx.YOSIDA)
    rp, ci = (np.asarray(x) for x in ora.graphs[0])
    n = len(rp) - 1
    F, lu = np.array(ora.matrix(0, 0)), np.array(ora.ilu_F())
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci
    bptr = a.dim * np.asarray(dofs.owned_u_ptr if a.ranks > 1 else [0, n // a.dim], dtype=np.int32)
    r32 = lambda v: v.astype(np.float32).astype(np.float64)
    lu32 = np.where(diag, lu, r32(lu))
    b = rng.standard_normal(n)
    nz = np.abs(F[F != 0])
    print("%d velocity DoF, %d ranks; |F| entries between %.2e and %.2e" % (n, len(bptr) - 1, nz.min(), nz.max()))
    x = rng.standard_normal(n)
    A64, A32 = sp.csr_matrix((F, ci, rp), shape=(n, n)), sp.csr_matrix((r32(F), ci, rp), shape=(n, n))
    print("one product differs by %.2e, one ILU application by %.2e (maximum norm, relative)"
          % (np.abs(A32 @ x - A64 @ x).max() / np.abs(A64 @ x).max(),
             np.abs(oracle.ilu0_solve(rp, ci, lu32, bptr, x) - oracle.ilu0_solve(rp, ci, lu, bptr, x)).max() / np.abs(oracle.ilu0_solve(rp, ci, lu, bptr, x)).max()))
    for rtol in (1e-2, 1e-6, 1e-10):
        counts = []
        for A, f in ((A64, lu), (A32, lu32)):
            it = [0]
            M = spla.LinearOperator((n, n), matvec=lambda v, f=f: oracle.ilu0_solve(rp, ci, f, bptr, v))
            spla.gmres(A, b, M=M, restart=28, rtol=rtol, atol=0.0, maxiter=100, callback=lambda r: it.__setitem__(0, it[0] + 1), callback_type="pr_norm")
            counts.append(it[0])
        print("rtol %.0e: inner iterations double / rounded = %d / %d" % (rtol, counts[0], counts[1]))


if __name__ == "__main__":
    main()
