#!/usr/bin/env python3
"""What one nsx_advect_tracers call costs on the problem bench.py times (the 1 089 643-DoF 3D cylinder as bench.py builds it: first-touch
numbering on one rank, 4096 virtual ranks laid out inside libnsx, Yosida, reference tolerances), behind a few solved steps so that
`solution` and `previous_solution` are those of a run.

  k_tracer_advect   RK4 with 4 substeps, fields FROZEN and LINEAR, 65 536 and 1 048 576 particles seeded uniformly in the bounding box:
                    microseconds per call between HIP events (launch scope "tracer_advect", nsx_profile_get).  Every timed call starts
                    from the same freshly seeded set (nsx_set_tracers is outside the events), so all calls move the same particles;
                    the counts of ACTIVE / EXITED / LOST particles behind a call are recorded beside its time.
  gather floor      k_probe_eval (launch scope "probe_eval") on 65 536 located points: its time per point x 16 evaluations (4 substeps x
                    4 stages) x particles -- one gather of a cell's nodal values per evaluation, no walk, no second state.
  scale             milliseconds per outer GMRES iteration of the same run (t_solve of the last step over its outer iterations).

Medians and the spread over the repeats go to profiles/tracers_timing.json.  No speed is claimed here: the file records what was measured.

    python tools/tracer_timing.py [--steps 3] [--repeats 10] [--level 7] [--ranks 4096] [--out profiles/tracers_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    v = sorted(float(x) for x in v)
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="time steps solved before the measurement")
    ap.add_argument("--repeats", type=int, default=10, help="timed calls per configuration (after one warm-up call)")
    ap.add_argument("--level", type=int, default=bench.BASE_LEVEL)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_timing.json"))
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
        result = {"dofs": int(dofs.n_dofs), "cells": int(dofs.n_cells), "level": args.level, "virtual_ranks": args.ranks, "steps_solved": args.steps,
                  "dt": bench.DT, "n_substeps": 4, "scheme": "RK4",
                  "outer_iterations_of_the_last_step": st["outer_iterations"], "t_solve_ms_of_the_last_step": 1e3 * st["t_solve"],
                  "ms_per_outer_iteration": 1e3 * st["t_solve"] / max(1, st["outer_iterations"])}
        V = np.asarray(mesh.vertices)
        lo, hi = V.min(axis=0), V.max(axis=0)
        cloud = lo + (hi - lo) * np.random.default_rng(7).random((1048576, 3))

        # ---- the gather floor: k_probe_eval on 65 536 points
        dev.set_probes(cloud[:65536])
        dev.eval_probes()
        dev.profile(True)
        dev.profile_reset()
        for _ in range(args.repeats):
            dev.eval_probes()
        tab = dev.profile_table()
        dev.profile(False)
        eval_us = 1e3 * tab["probe_eval"]["total_ms"] / tab["probe_eval"]["launches"]
        result["probe_eval"] = {"points": 65536, "us_per_launch": eval_us, "ns_per_point": 1e3 * eval_us / 65536, "launches": tab["probe_eval"]["launches"]}
        dev.set_probes(np.zeros((0, 3)))

        # ---- k_tracer_advect
        result["advect"] = {}
        for n in (65536, 1048576):
            for field, fname in ((nsx.TRACER_FROZEN, "frozen"), (nsx.TRACER_LINEAR, "linear")):
                times = []
                for rep in range(args.repeats + 1):
                    dev.set_tracers(cloud[:n])
                    dev.profile(True)
                    dev.profile_reset()
                    dev.advect_tracers(bench.DT, 4, nsx.TRACER_RK4, field)
                    tab = dev.profile_table()
                    dev.profile(False)
                    if rep:                          # the first call is the warm-up
                        times.append(1e3 * tab["tracer_advect"]["total_ms"] / tab["tracer_advect"]["launches"])
                status = dev.get_tracers()["status"]
                s = summary(times)
                floor_us = 16 * n * result["probe_eval"]["ns_per_point"] * 1e-3
                result["advect"]["%s_%d" % (fname, n)] = dict(
                    s, particles=n, field=fname, algorithmic_bytes_per_launch=tab["tracer_advect"]["bytes_per_launch"],
                    not_found=int((status == nsx.TRACER_NOT_FOUND).sum()), active=int((status == nsx.TRACER_ACTIVE).sum()),
                    exited=int((status == nsx.TRACER_EXITED).sum()), lost=int((status == nsx.TRACER_LOST).sum()),
                    gather_floor_us=floor_us, median_over_gather_floor=s["median_us"] / floor_us if floor_us > 0 else None,
                    median_in_outer_iterations=1e-3 * s["median_us"] / result["ms_per_outer_iteration"])
        result["advect_of_65536_costs_less_than_one_outer_iteration"] = bool(
            max(result["advect"][k]["max_us"] for k in ("frozen_65536", "linear_65536")) * 1e-3 < result["ms_per_outer_iteration"])
    finally:
        dev.close()
    text = json.dumps(result, indent=1)
    if args.out and args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"ms_per_outer_iteration": result["ms_per_outer_iteration"], "probe_eval_ns_per_point": result["probe_eval"]["ns_per_point"],
                      "advect_median_us": {k: v["median_us"] for k, v in result["advect"].items()},
                      "less_than_one_outer_iteration": result["advect_of_65536_costs_less_than_one_outer_iteration"]}))


if __name__ == "__main__":
    main()
