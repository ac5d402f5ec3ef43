"""Worker of tests/test_gpu_probes.py::test_distributed_probes_have_one_owner_and_every_rank_the_same_values (launched with
torch.distributed.run, gloo backend; built like tests/diagnostics_dist_worker.py): every rank holds one handle on cuda:0 and exchanges through
host callbacks.  No solve runs here: the only collectives are those of the two probe calls.  Every rank writes what IT got -- cells, owners,
lambda, found, the values, the global ids of its view's cells and its collective counters around the two calls -- into a file of its own.
points() and state() are shared with the test, which runs the single-process handle on the same input.

    python -m torch.distributed.run ... tests/probes_dist_worker.py DIM LEVEL N_SUB OUT_PREFIX
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


def points(mesh, dofs, world, n_shared=50):
    """the recipe of the parity test plus n_shared P2 nodes that lie in layer-1 cells of both of the first two ranks (taken from the two
    views' cell_ids): (points, slices by name)"""
    import probe_reference as PR
    dim = mesh.dim
    nv = dim + 1
    np2 = 6 if dim == 2 else 10
    base = [(dim + 1) * a if a < nv else nv * (dim + 1) + dim * (a - nv) for a in range(np2)]
    cd = np.asarray(dofs.cell_dofs)
    nodes = []
    for r in range(2):
        v = dofs.rank_view(r, world)
        nodes.append(np.unique(cd[v["cell_ids"][:v["n_cells_layer1"]]][:, base] // dim))
    both = np.intersect1d(nodes[0], nodes[1])
    pick = np.sort(np.random.default_rng(13).choice(both, size=n_shared, replace=False))
    shared = np.asarray(dofs.support_points)[pick * dim].copy()
    parts = [("uniform", PR.box_points(mesh, 200)), ("support", PR.support_points(dofs, 200)), ("pressure", PR.pressure_points(dim)),
             ("outside", PR.outside_points(dim)), ("shared", shared)]
    where, s = {}, 0
    for name, x in parts:
        where[name] = slice(s, s + len(x))
        s += len(x)
    return np.concatenate([x for _, x in parts]), where


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
    dev.set_solution(state(dofs))
    pts, _ = points(mesh, dofs, world)
    before = dev.comm_counters()
    dev.set_probes(pts)                                  # the points go in unchanged, the same on every rank
    mid = dev.comm_counters()
    ev = dev.eval_probes(gradient=True)
    after = dev.comm_counters()
    cells, owners, lam = dev.probe_cells()
    np.savez("%s_rank%d.npz" % (out_prefix, rank), rank=rank, world=world, cells=cells, owners=owners, lam=lam, found=ev["found"],
             velocity=ev["velocity"], pressure=ev["pressure"], gradient=ev["gradient"], cell_ids=dev.view["cell_ids"],
             n_layer1=dev.view["n_cells_layer1"], counters=np.array([before, mid, after]))
    faulthandler.cancel_dump_traceback_later()
    dev.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
