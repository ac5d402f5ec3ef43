#!/usr/bin/env python3
"""What a call of the flow diagnostics (include/nsx.h: nsx_compute_diagnostics) costs on the bench mesh, against its yardstick from the
same process: the scope of k_cell_convection in one assemble_time_step -- the per-step cell kernel it is built like (it gathers one
vector where k_cell_diag gathers two, and stores 100 doubles per cell where k_cell_diag stores 8).

The problem is built the way bench.py builds its default one (3D cylinder level 7, 1 089 643 DoF, 246 336 cells, first-touch numbering
on one rank, 4096 virtual ranks in colour order built inside libnsx, Schur ILU blocks of at most 96 rows); one time step prepares a state
with a non-zero previous_solution.  Then, with the per-scope HIP-event timer on: one assemble_time_step, 5 warm-up calls of
diagnostics() and 20 timed ones.  Prints the mean microseconds of diag_cells and diag_reduce, the wall time per call (host round trip
included) and the cell_convection scope; --out writes them as JSON.  A tool, not a test; needs the GPU.

    python tools/diagnostics_probe.py [--level 7] [--ranks 4096] [--calls 20] [--warmup 5] [--out profiles/diagnostics_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU, DT, SCHUR_ROWS = 1e-3, 2e-4, 96
STEP_MS = 70.0  # one time step of the bench workload, for the percentage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh = Mesh.cylinder(3, a.level).partition(1, 1)
    dofs, tables = DoFs(mesh, "first_touch"), Tables(3)
    dev = nsx.Nsx(dofs, tables, NU, DT, layout=(a.ranks, nsx.COLOUR, SCHUR_ROWS))
    try:
        inlet = InletVelocity(3)
        dev.set_solution(np.zeros(dofs.n_dofs))
        dev.assemble(nsx.TEMAM)
        dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, DT))
        st = dev.solve_time_step(nsx.YOSIDA)
        dev.profile(True)
        dev.profile_reset()
        dev.assemble_time_step(0)
        for _ in range(a.warmup):
            dev.diagnostics()
        conv = dev.profile_table()["cell_convection"]
        dev.profile_reset()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            d = dev.diagnostics()
        wall_us = (time.perf_counter() - t0) / a.calls * 1e6
        table = dev.profile_table()
        dev.profile(False)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            dev.diagnostics()
        wall_plain_us = (time.perf_counter() - t0) / a.calls * 1e6
    finally:
        dev.close()

    def scope(e):
        us = e["total_ms"] / e["launches"] * 1e3
        return {"launches": e["launches"], "mean_us": us, "alg_GBps": e["bytes_per_launch"] / us * 1e-3, "percent_of_a_%g_ms_step" % STEP_MS: us / (10.0 * STEP_MS)}

    res = {"what": "nsx_compute_diagnostics on the 3D cylinder level %d: %d DoF, %d cells, %d virtual ranks; %d calls after %d warm-up calls"
                   % (a.level, dofs.n_dofs, dofs.n_cells, a.ranks, a.calls, a.warmup),
           "outer_iterations_of_the_preparing_step": st["outer_iterations"],
           "diag_cells": scope(table["diag_cells"]), "diag_reduce": scope(table["diag_reduce"]),
           "cell_convection_same_process": scope(conv),
           "wall_us_per_call_profile_on": wall_us, "wall_us_per_call": wall_plain_us,
           "wall_percent_of_a_%g_ms_step" % STEP_MS: wall_plain_us / (10.0 * STEP_MS),
           "diagnostics": d}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
