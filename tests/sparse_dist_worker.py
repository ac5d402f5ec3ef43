"""Worker of tests/test_gpu_sparse.py::test_distributed_products (launched with torch.distributed.run, gloo backend; built like
tests/dist_worker.py): every rank holds one handle on cuda:0, exchanges through host callbacks, and runs every op of nsx_sparse_product
on the vectors the parent prepared (the seeded normal x, and x = 0); the owned entries of every result are all-reduced, and rank 0 saves
them with what every rank's handle says about the path each op took (nsx_path_info and the profile scopes it opened).  The switches
(NSX_SPMV_BLOCKED, NSX_INNER_PRECISION) come through the environment, as for every program that sets them before it creates its handles.

    python -m torch.distributed.run ... tests/sparse_dist_worker.py DIM LEVEL N_SUB IN.npz OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCOPES = ("spmv_F", "spmv_F_if", "halo_u_wait", "spmv_B", "spmv_G", "spmv_S", "spmv_saddle_u", "spmv_saddle_if", "halo_up_wait")


def main():
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=False)  # a rank that is still here after two minutes says where it is stuck
    import torch
    import torch.distributed as dist
    import sparse_reference as R
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
    dev.prec_initialize(nsx.YOSIDA)
    dev.profile(True)
    x, aux = inp["x"], inp["aux"]
    vecs = (x, np.zeros_like(x))
    ys = np.zeros((len(R.OPS), len(vecs), dofs.n_dofs))
    infos = np.zeros((len(R.OPS), world, 32), dtype=np.int64)
    scopes = np.zeros((len(R.OPS), world, len(SCOPES)), dtype=np.int64)
    keys = None
    for oi, op in enumerate(R.OPS):
        for vi, v in enumerate(vecs):
            dev.profile_reset()
            y = dev.sparse_product(oi, v, aux if op in R.NEEDS_AUX else None)      # owned entries, zeros elsewhere
            table = dev.profile_table()
            info = dev.path_info()
            t = torch.from_numpy(y)
            dist.all_reduce(t)
            ys[oi, vi] = t.numpy()
        keys = list(info.keys())
        infos[oi, rank] = list(info.values())
        scopes[oi, rank] = [table.get(s, {}).get("launches", 0) for s in SCOPES]
    for a in (infos, scopes):
        dist.all_reduce(torch.from_numpy(a))
    if rank == 0:
        np.savez(out, y=ys, path_keys=np.array(keys), path_info=infos, scope_names=np.array(SCOPES), scopes=scopes)
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
