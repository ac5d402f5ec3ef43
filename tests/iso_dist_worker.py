"""Worker of tests/test_gpu_isosurface.py::test_distributed_extraction_is_the_single_process_surface_cell_by_cell (launched with
torch.distributed.run, gloo backend; built like tests/nodal_dist_worker.py): every rank holds one handle on cuda:0 and exchanges through host
callbacks.  No solve runs here and the extraction issues no collective.  Every rank writes what IT got -- its primitives for every case of
cases(), the global ids of its view's cells, its collective counters around the calls and the return code of an NSX_ISO_NODAL request -- into a
file of its own.  state() and cases() are shared with the test, which runs the single-process handle on the same input.

    python -m torch.distributed.run ... tests/iso_dist_worker.py DIM LEVEL N_SUB OUT_PREFIX
"""
import ctypes
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


def cases(nsx):
    """(name, field, isovalue, colour)"""
    S = nsx.iso_source
    return [("speed", S(nsx.ISO_VELOCITY, component=-1), 0.35, S(nsx.ISO_PRESSURE)),
            ("slice", S(nsx.ISO_PLANE, normal=[1.0, 0.3, 0.2]), 1.234, S(nsx.ISO_VELOCITY, component=0)),
            ("pressure", S(nsx.ISO_PRESSURE), None, None)]             # None: the middle of the pressure's range


def isovalue(name, iso, dofs, u):
    return iso if iso is not None else float(0.5 * (u[dofs.n_u:].min() + u[dofs.n_u:].max()) + 1e-3)


def main():
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=False)  # a rank that is still here after two minutes says where it is stuck
    import torch.distributed as dist
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    dim, level, n_sub, out_prefix = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    dt = 2e-4 if dim == 3 else 1e-2
    dev = nsx.Nsx(dofs, tables, 1e-3, dt, device=0, rank=rank, world=world, comm="callbacks")
    u = state(dofs)
    dev.set_solution(u)
    out = {}
    before = dev.comm_counters()
    for name, field, iso, colour in cases(nsx):
        pts, col, cells = dev.extract_isosurface(field, isovalue(name, iso, dofs, u), colour)
        out[name + "_points"], out[name + "_cells"] = pts, cells
        if col is not None:
            out[name + "_colour"] = col
    mid = dev.comm_counters()
    # NSX_ISO_NODAL is refused across processes, as field and as colour, with or without nodal results; the last result stays readable
    n = ctypes.c_int64(-7)
    nodal = nsx.iso_source(nsx.ISO_NODAL, which=nsx.FIELD_Q)
    rcs = [dev.L.nsx_extract_isosurface(dev._h, ctypes.byref(nodal), 0.0, None, ctypes.byref(n))]
    dev.compute_nodal_fields()
    rcs.append(dev.L.nsx_extract_isosurface(dev._h, ctypes.byref(nodal), 0.0, None, ctypes.byref(n)))
    rcs.append(dev.L.nsx_extract_isosurface(dev._h, ctypes.byref(nsx.iso_source(nsx.ISO_PRESSURE)), 0.0, ctypes.byref(nodal), ctypes.byref(n)))
    kept = np.empty_like(out["pressure_points"])
    rcs.append(dev.L.nsx_get_isosurface(dev._h, kept.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None))
    after = dev.comm_counters()
    np.savez("%s_rank%d.npz" % (out_prefix, rank), rank=rank, world=world, cell_ids=dev.view["cell_ids"], n_layer1=dev.view["n_cells_layer1"],
             counters=np.array([before, mid, after]), nodal_rc=np.array(rcs), n_after_refusal=n.value, kept=kept, **out)
    faulthandler.cancel_dump_traceback_later()
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
