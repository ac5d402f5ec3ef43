"""Worker of tests/test_gpu_diagnostics.py::test_distributed_diagnostics_count_every_cell_once (launched with torch.distributed.run, gloo
backend; built like tests/inner_precision_dist_worker.py): every rank holds one handle on cuda:0 and exchanges through host callbacks.
No solve runs here: the only collectives are those of the diagnostics call.  Every rank writes what IT got -- the totals, its per-cell
planes, the global ids of its view's cells and its collective counters around the call -- into a file of its own.

    python -m torch.distributed.run ... tests/diagnostics_dist_worker.py DIM LEVEL N_SUB OUT_PREFIX
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=False)  # a rank that is still here after two minutes says where it is stuck
    import torch.distributed as dist
    import diagnostics_reference as R
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    dim, level, n_sub, out_prefix = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    dt = 2e-4 if dim == 3 else 1e-2
    dev = nsx.Nsx(dofs, tables, 1e-3, dt, device=0, rank=rank, world=world, comm="callbacks")
    dev.set_solution(R.smooth_field(dofs))
    before = dev.comm_counters()
    d = dev.diagnostics()
    after = dev.comm_counters()
    cells = np.array([dev.cell_diagnostic(w) for w in range(nsx.DIAG_COUNT)])
    keys = sorted(d)
    np.savez("%s_rank%d.npz" % (out_prefix, rank), rank=rank, world=world, keys=np.array(keys), totals=np.array([float(d[k]) for k in keys]),
             cells=cells, cell_ids=dev.view["cell_ids"], n_layer1=dev.view["n_cells_layer1"], counters=np.array([before, after]))
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
