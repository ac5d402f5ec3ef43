"""Worker of tests/test_gpu_tracers.py::test_distributed_handles_refuse_tracers_without_a_collective (launched with torch.distributed.run,
gloo backend; built like tests/probes_dist_worker.py): every rank holds one handle on cuda:0 and exchanges through host callbacks.  The three
tracer calls are made raw, their return codes and the collective counters around them go into a file per rank.

    python -m torch.distributed.run ... tests/tracers_dist_worker.py DIM LEVEL OUT_PREFIX
"""
import ctypes
import json
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
    import probe_reference as PR
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    dim, level, out_prefix = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mesh = Mesh.cylinder(dim, level).partition(world, 1)
    dofs, tables = DoFs(mesh), Tables(dim)
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4 if dim == 3 else 1e-2, device=0, rank=rank, world=world, comm="callbacks")
    dev.set_solution(R.smooth_field(dofs))
    pts = np.ascontiguousarray(PR.box_points(mesh, 20, seed=5))
    f64p = ctypes.POINTER(ctypes.c_double)
    before = dev.comm_counters()
    rc = {"set": dev.L.nsx_set_tracers(dev._h, len(pts), pts.ctypes.data_as(f64p), -1.0)}
    message = (dev.L.nsx_last_error(dev._h) or b"").decode()
    rc["advect"] = dev.L.nsx_advect_tracers(dev._h, 0.1, 4, 4, 0)
    rc["get"] = dev.L.nsx_get_tracers(dev._h, None, None, None, None, None)
    after = dev.comm_counters()
    dev.set_probes(pts)                                  # a collective call that every rank makes: the handle works
    found = int(dev.eval_probes()["found"].sum())
    with open("%s_rank%d.json" % (out_prefix, rank), "w") as f:
        json.dump({"rank": rank, "world": world, "rc": rc, "message": message, "before": list(before), "after": list(after), "probes_found": found}, f)
    faulthandler.cancel_dump_traceback_later()
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
