"""Worker of tests/test_gpu_schur_cg.py::test_two_processes_iterates (launched with torch.distributed.run, gloo backend; built like
tests/dist_worker.py): every rank holds one handle on cuda:0, exchanges through host callbacks, and runs nsx_schur_cg with rtol = 0,
maxiter = k from the guesses the parent prepared; the owned entries of every iterate are all-reduced and rank 0 saves them with what the
handle says about the path it took.

    python -m torch.distributed.run ... tests/schur_cg_dist_worker.py N_SUB SCHUR_MERGE IN.npz OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=False)  # a rank that is still here after two minutes says where it is stuck
    import torch
    import torch.distributed as dist
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    n_sub, merge, inp, out = int(sys.argv[1]), int(sys.argv[2]), np.load(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mesh = Mesh.cylinder(3, 1).partition(world, n_sub)
    dofs, tables = DoFs(mesh, "colour"), Tables(3)
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4, device=0, rank=rank, world=world, comm="callbacks")
    dev.set_schur_blocks(np.ascontiguousarray(dofs.owned_p_ptr[rank * n_sub:(rank + 1) * n_sub + 1][::merge]))
    dev.set_solution(0.05 * np.random.default_rng(5).standard_normal(dofs.n_dofs))
    dev.assemble(nsx.TEMAM)
    dev.apply_boundary_values(*cylinder_boundary_values(dofs, InletVelocity(3, 2), 2e-4))
    dev.prec_initialize(nsx.YOSIDA)
    dev.profile(True)
    ks = [int(k) for k in inp["ks"]]
    guesses = ("zero", "visible")
    xs = np.zeros((len(guesses), len(ks), dofs.n_p))
    steps, status = np.zeros((len(guesses), len(ks)), dtype=np.int64), np.zeros((len(guesses), len(ks)), dtype=np.int64)
    last = np.zeros((len(guesses), len(ks)))
    for gi, guess in enumerate(guesses):
        for ki, k in enumerate(ks):
            x, steps[gi, ki], last[gi, ki], status[gi, ki] = dev.schur_cg(inp["b"], inp[guess], rtol=0.0, maxiter=k)
            t = torch.from_numpy(x)          # owned entries, zeros elsewhere
            dist.all_reduce(t)
            xs[gi, ki] = t.numpy()
    info = dev.path_info()
    scopes = sorted(k for k, v in dev.profile_table().items() if v["launches"] > 0)
    if rank == 0:
        np.savez(out, x=xs, steps=steps, last=last, status=status, scopes=np.array(scopes), path_keys=np.array(list(info.keys())),
                 path_info=np.array(list(info.values())))
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
