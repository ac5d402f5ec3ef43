"""Launch times of the surface-load kernels (csrc/nsx_surface.hip) on the bench mesh with ALL boundary faces in 4 groups: the HIP-event
scopes surface_faces, surface_nodes and surface_fold of nsx_profile_get, warm, averaged over the launches of two rounds, and the host clock
around a whole nsx_compute_surface with totals.  Prints one JSON line.  DESIGN.md section 5 quotes it.

    python tools/surface_timing.py [--level 7] [--calls 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import boundary_faces
    mesh = Mesh.cylinder(3, a.level)
    dofs, tables = DoFs(mesh), Tables(3)
    cells, lfs, groups = boundary_faces(mesh)
    X = np.asarray(dofs.support_points)
    u = np.zeros(dofs.n_dofs)
    u[:dofs.n_u] = np.sin(3 * X[:dofs.n_u, 0] + np.arange(dofs.n_u) % 3) * X[:dofs.n_u, 1]
    u[dofs.n_u:] = X[dofs.n_u:, 0]
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4)
    out = {"level": a.level, "n_cells": int(dofs.n_cells), "n_dofs": int(dofs.n_dofs), "n_faces": int(len(cells)),
           "group_sizes": np.bincount(groups).tolist(), "calls": a.calls, "rounds": []}
    try:
        dev.set_solution(u)
        dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, [0.5, 0.2, 0.205])
        out["n_surface_nodes"] = dev.surface_info()["n_nodes"]
        for _ in range(5):
            dev.compute_surface()
        for _ in range(2):
            dev.profile(True)
            dev.profile_reset()
            for _ in range(a.calls):
                dev.compute_surface()
            table = dev.profile_table()
            dev.profile(False)
            t0 = time.perf_counter()
            for _ in range(a.calls):
                dev.compute_surface()
            wall = (time.perf_counter() - t0) / a.calls
            out["rounds"].append({"wall_us_per_call": 1e6 * wall,
                                  **{k: {"us_per_launch": 1e3 * v["total_ms"] / max(1, v["launches"]), "launches": v["launches"],
                                         "bytes_per_launch": v["bytes_per_launch"]}
                                     for k, v in table.items() if k.startswith("surface_")}})
    finally:
        dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
