"""Worker of tests/test_gpu_nodal_fields.py::test_distributed_nodal_fields_equal_the_single_process_handles_bitwise (launched with
torch.distributed.run, gloo backend; built like tests/probes_dist_worker.py): every rank holds one handle on cuda:0 and exchanges through
host callbacks.  No solve runs here and the nodal-field calls issue no collective.  Every rank writes what IT got -- the five fields
(global-sized, its owned entries filled), the ownership ranges, the global ids of its view's cells and its collective counters around the
calls -- into a file of its own.  state() is shared with the test, which runs the single-process handle on the same input.

    python -m torch.distributed.run ... tests/nodal_dist_worker.py DIM LEVEL N_SUB OUT_PREFIX
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def state(dofs):
    """a state that depends on the position of a node only: smooth velocity, linear pressure"""
    import diagnostics_reference as R
    import probe_reference as PR
    return R.smooth_field(dofs) + PR.linear_pressure(dofs)


def main():
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=False)  # a rank that is still here after two minutes says where it is stuck
    import torch.distributed as dist
    import nodal_reference as NR
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    dim, level, n_sub, out_prefix = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    dt = 2e-4 if dim == 3 else 1e-2
    dev = nsx.Nsx(dofs, tables, 1e-3, dt, device=0, rank=rank, world=world, comm="callbacks")
    dev.set_solution(state(dofs))
    before = dev.comm_counters()
    dev.compute_nodal_fields()
    mid = dev.comm_counters()
    got = {name: dev.nodal_field(k) for k, name in enumerate(NR.NAMES)}
    after = dev.comm_counters()
    np.savez("%s_rank%d.npz" % (out_prefix, rank), rank=rank, world=world, gpu_u_ptr=dev.view["gpu_u_ptr"], cell_ids=dev.view["cell_ids"],
             n_layer1=dev.view["n_cells_layer1"], counters=np.array([before, mid, after]), **got)
    faulthandler.cancel_dump_traceback_later()
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
