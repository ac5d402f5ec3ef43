"""Worker of tests/test_gpu_inner_precision.py::test_distributed_solve_in_fp32_equals_single_process_in_fp32 (launched with
torch.distributed.run, gloo backend; built like tests/dist_worker.py): every rank holds one handle on cuda:0, exchanges through host
callbacks and writes what IT saw -- its path info and its profile scopes after every step -- into a file of its own, so that the test can
assert on every rank; rank 0 also writes the gathered solutions and iteration counts.  The inner precision comes from the environment
(NSX_INNER_PRECISION), as for every program that does not call nsx_set_inner_precision itself.

    python -m torch.distributed.run ... tests/inner_precision_dist_worker.py DIM LEVEL N_SUB PREC OUT_PREFIX ORDERING
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=False)  # a rank that is still here after two minutes says where it is stuck
    import torch.distributed as dist
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    dim, level, n_sub, prec = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    out_prefix, ordering = sys.argv[5], sys.argv[6]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh, ordering), Tables(dim)
    dt = 2e-4 if dim == 3 else 1e-2
    dev = nsx.Nsx(dofs, tables, 1e-3, dt, device=0, rank=rank, world=world, comm="callbacks")
    inlet = InletVelocity(dim, 2 if dim == 3 else 3)
    u0 = 0.05 * np.random.default_rng(5).standard_normal(dofs.n_dofs)
    dev.set_solution(u0)
    iters, sols, infos = [], [], []
    t = 0.0
    dev.profile(True)
    for step in range(3):
        t += dt
        if step == 0:
            dev.assemble(nsx.TEMAM)
        else:
            dev.assemble_time_step(nsx.TEMAM if dim == 2 else 0)
        dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, t))
        st = dev.solve_time_step(prec, tol_abs=1e-10, inner_rtol=1e-10)
        iters.append(st["outer_iterations"])
        sols.append(dev.gather_solution())
        infos.append(list(dev.path_info().values()))     # this rank's paths in the step it has just solved
    table = dev.profile_table()
    scopes = sorted(k for k, v in table.items() if v["launches"] > 0)
    np.savez("%s_rank%d.npz" % (out_prefix, rank), rank=rank, world=world, path_keys=np.array(list(nsx.Nsx.PATH_KEYS)), path_info=np.array(infos),
             scopes=np.array(scopes), scope_launches=np.array([table[k]["launches"] for k in scopes]),
             scope_bytes=np.array([table[k]["bytes_per_launch"] for k in scopes]), iters=np.array(iters),
             **({"sols": np.array(sols), "u0": u0} if rank == 0 else {}))
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
