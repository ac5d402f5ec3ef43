#!/usr/bin/env python3
"""What one nsx_compute_nodal_fields call costs on the problem bench.py times (the 1 089 643-DoF 3D cylinder as bench.py builds it:
first-touch numbering on one rank, 4096 virtual ranks laid out inside libnsx, Yosida, reference tolerances), behind a few solved steps so
that `solution` is that of a run.

  k_nodal_fields    microseconds per call between HIP events (launch scope "nodal_fields", nsx_profile_get), the first call (which builds
                    and uploads the patch table) outside the timed ones; the wall time of that first call is recorded beside it.
  floor             the wall time of nsx_get_solution_ghosted on the same handle: what any host-side alternative pays before it has
                    looked at a single cell.  The wall time of one nsx_get_nodal_field (the download of one field) stands beside it.
  share of HBM      the launch's algorithmic bytes (csrc/nsx_nodal.hip: every operand once) over its time, as a fraction of the HBM copy
                    rate (6.29 TB/s measured for a float4 copy on this chip).
  scale             milliseconds per outer GMRES iteration of the same run.

Medians and the spread over the repeats go to profiles/nodal_fields_timing.json.  No speed is claimed here: the file records what was measured.

    python tools/nodal_fields_timing.py [--steps 3] [--repeats 20] [--level 7] [--ranks 4096] [--out profiles/nodal_fields_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_BYTES_PER_S = 6.29e12


def summary(v):
    v = sorted(float(x) for x in v)
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="time steps solved before the measurement")
    ap.add_argument("--repeats", type=int, default=20, help="timed calls (after the first call, which builds the patch table)")
    ap.add_argument("--level", type=int, default=bench.BASE_LEVEL)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nodal_fields_timing.json"))
    args = ap.parse_args()
    args.numbering, args.ordering, args.schur_blocks = "first_touch", "colour", 0   # bench.py's defaults

    import numpy as np
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh, dofs, tables = bench.build_problem(args.level, args.ranks, numbering="first_touch", ranks_input=1)
    dev = nsx.Nsx(dofs, tables, bench.NU, bench.DT, layout=bench.layout_of(args, dofs))
    try:
        dev.set_solution(np.zeros(dofs.n_dofs))
        inlet = InletVelocity(3)
        for step in range(args.steps):
            if step == 0:
                dev.assemble(nsx.TEMAM)
            else:
                dev.assemble_time_step(nsx.TEMAM)
            dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, (step + 1) * bench.DT))
            st = dev.solve_time_step(nsx.YOSIDA)
        result = {"dofs": int(dofs.n_dofs), "cells": int(dofs.n_cells), "p2_nodes": int(dofs.n_u // 3), "level": args.level,
                  "virtual_ranks": args.ranks, "steps_solved": args.steps,
                  "ms_per_outer_iteration": 1e3 * st["t_solve"] / max(1, st["outer_iterations"])}
        t0 = time.perf_counter()
        dev.compute_nodal_fields()                       # builds the patch table
        result["first_call_with_table_build_ms"] = 1e3 * (time.perf_counter() - t0)
        times = []
        for _ in range(args.repeats):
            dev.profile(True)
            dev.profile_reset()
            dev.compute_nodal_fields()
            tab = dev.profile_table()
            dev.profile(False)
            times.append(1e3 * tab["nodal_fields"]["total_ms"] / tab["nodal_fields"]["launches"])
        s = summary(times)
        nbytes = tab["nodal_fields"]["bytes_per_launch"]
        result["compute"] = dict(s, algorithmic_bytes_per_launch=nbytes, bytes_per_s_at_median=nbytes / (1e-6 * s["median_us"]),
                                 fraction_of_hbm_copy_rate=nbytes / (1e-6 * s["median_us"]) / HBM_COPY_BYTES_PER_S)

        def wall(f):
            v = []
            for _ in range(args.repeats):
                t = time.perf_counter()
                f()
                v.append(1e6 * (time.perf_counter() - t))
            return summary(v)
        buf = np.empty(dofs.n_dofs)
        ptr = buf.ctypes.data_as(nsx._f64p)
        rcs = []
        result["get_solution_ghosted_wall"] = wall(lambda: rcs.append(dev.L.nsx_get_solution_ghosted(dev._h, ptr)))
        if any(rcs) or not np.array_equal(buf, dev.solution):
            raise RuntimeError("nsx_get_solution_ghosted failed or returned another vector")
        result["get_solution_ghosted_bytes"] = int(buf.nbytes)
        result["get_nodal_field_q_wall"] = wall(lambda: dev.nodal_field(nsx.FIELD_Q))
        result["get_nodal_field_gradient_wall"] = wall(lambda: dev.nodal_field(nsx.FIELD_GRADIENT))
        w = dev.nodal_field(nsx.FIELD_VORTICITY)
        result["vorticity_nonzero_fraction"] = float((np.abs(w).max(axis=1) > 0).mean())
        result["all_finite"] = bool(np.isfinite(w).all())
        result["compute_over_download_floor"] = s["median_us"] / result["get_solution_ghosted_wall"]["median_us"]
    finally:
        dev.close()
    text = json.dumps(result, indent=1)
    if args.out and args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"compute_median_us": s["median_us"], "fraction_of_hbm_copy_rate": result["compute"]["fraction_of_hbm_copy_rate"],
                      "get_solution_ghosted_median_us": result["get_solution_ghosted_wall"]["median_us"],
                      "first_call_ms": result["first_call_with_table_build_ms"], "ms_per_outer_iteration": result["ms_per_outer_iteration"]}))


if __name__ == "__main__":
    main()
