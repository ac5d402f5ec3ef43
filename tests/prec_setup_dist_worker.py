"""Worker of tests/test_gpu_prec_setup.py::test_distributed_schur_columns (launched with torch.distributed.run, gloo backend; built like
tests/sparse_dist_worker.py): every rank holds one handle on cuda:0 and exchanges through host callbacks.  For every preconditioner type
the parent names: nsx_prec_initialize, the set-up vectors (nsx_prec_get_vector: owned entries, zeros elsewhere) and the S op of
nsx_sparse_product on the unit vectors of the pressure dofs the parent chose, all of them all-reduced; rank 0 saves them with the
launches of the set-up's profile scopes on every rank.

    python -m torch.distributed.run ... tests/prec_setup_dist_worker.py DIM LEVEL N_SUB IN.npz OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCOPES = ("extract_diag", "abs_rowsum", "schur_numeric", "ilu_factor_S", "spmv_S")


def main():
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=False)  # a rank that is still here after two minutes says where it is stuck
    import torch
    import torch.distributed as dist
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    dim, level, n_sub, inp, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), np.load(sys.argv[4]), sys.argv[5]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh, "first_touch"), Tables(dim)
    dt = 2e-4 if dim == 3 else 1e-2
    dev = nsx.Nsx(dofs, tables, 1e-3, dt, device=0, rank=rank, world=world, comm="callbacks")
    dev.set_solution(inp["u0"])
    dev.assemble(nsx.TEMAM)
    dev.apply_boundary_values(*cylinder_boundary_values(dofs, InletVelocity(dim, 2), dt))
    dev.profile(True)
    types, picks = [int(t) for t in inp["types"]], [int(j) for j in inp["picks"]]
    vecs = np.zeros((len(types), nsx.PREC_VEC_COUNT, dofs.n_u))
    cols = np.zeros((len(types), len(picks), dofs.n_dofs))
    scopes = np.zeros((len(types), world, len(SCOPES)), dtype=np.int64)
    for ti, t in enumerate(types):
        dev.profile_reset()
        dev.prec_initialize(t)
        for which in range(nsx.PREC_VEC_COUNT):
            vecs[ti, which] = dev.prec_vector(which)
        for k, j in enumerate(picks):
            e = np.zeros(dofs.n_dofs)
            e[dofs.n_u + j] = 1.0
            cols[ti, k] = dev.sparse_product(nsx.PROD_S, e)
        table = dev.profile_table()
        scopes[ti, rank] = [table.get(s, {}).get("launches", 0) for s in SCOPES]
    for a in (vecs, cols, scopes):
        dist.all_reduce(torch.from_numpy(a))
    if rank == 0:
        np.savez(out, vectors=vecs, columns=cols, scope_names=np.array(SCOPES), scopes=scopes)
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
