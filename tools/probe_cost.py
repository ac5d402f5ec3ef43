#!/usr/bin/env python3
"""What the per-step pressure difference costs, measured two ways on the problem bench.py times (the 1 089 643-DoF 3D cylinder as bench.py
builds it: first-touch numbering on one rank, 4096 virtual ranks laid out inside libnsx, Yosida, reference tolerances):

  A  the host path: nsx_get_solution (the whole vector comes down) + DoFs.pressure_difference (nsxh_pressure_difference searches the cell
     list on the host) -- what the mirror's compute_pressure_difference does;
  B  the device path: nsx_eval_probes on the two pressure points, located once by nsx_set_probes (include/nsx.h, section "point probes").

After one solved step A and B ALTERNATE call by call in ONE process on one handle -- the same state, the same clocks, the same neighbours on
the card; every call ends in a synchronised copy, so a host clock around it measures the whole call.  The set-up cost of B (nsx_set_probes:
one pass of k_probe_locate over the cells) is timed for 2, 256 and 4096 points.  Medians and the run-to-run spread go to
profiles/probes_cost.json; no factor is claimed that is not more than 3 x the spread.

    python tools/probe_cost.py [--repeats 20] [--level 7] [--ranks 4096] [--out profiles/probes_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    v = sorted(float(x) for x in v)
    return {"median_ms": statistics.median(v), "min_ms": v[0], "max_ms": v[-1], "spread_ms": v[-1] - v[0],
            "iqr_ms": v[(3 * len(v)) // 4] - v[len(v) // 4], "n": len(v)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20, help="timed calls of A and of B (alternating), at least 10")
    ap.add_argument("--level", type=int, default=bench.BASE_LEVEL)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probes_cost.json"))
    args = ap.parse_args()
    args.repeats = max(10, args.repeats)
    args.numbering, args.ordering, args.schur_blocks = "first_touch", "colour", 0   # bench.py's defaults

    import numpy as np
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh, dofs, tables = bench.build_problem(args.level, args.ranks, numbering="first_touch", ranks_input=1)
    a, b = np.array([0.45, 0.2, 0.205]), np.array([0.55, 0.2, 0.205])
    dev = nsx.Nsx(dofs, tables, bench.NU, bench.DT, layout=bench.layout_of(args, dofs))
    try:
        dev.set_solution(np.zeros(dofs.n_dofs))
        dev.assemble(nsx.TEMAM)
        dev.apply_boundary_values(*cylinder_boundary_values(dofs, InletVelocity(3), bench.DT))
        st = dev.solve_time_step(nsx.YOSIDA)
        result = {"dofs": int(dofs.n_dofs), "cells": int(dofs.n_cells), "level": args.level, "virtual_ranks": args.ranks,
                  "outer_iterations_of_the_step": st["outer_iterations"], "solution_bytes": 8 * int(dofs.n_dofs)}

        # ---- set-up: nsx_set_probes for 2, 256 and 4096 points (the two pressure points first, then uniform points of the bounding box)
        V = np.asarray(mesh.vertices)
        lo, hi = V.min(axis=0), V.max(axis=0)
        cloud = np.concatenate([[a, b], lo + (hi - lo) * np.random.default_rng(7).random((4094, 3))])
        result["set_probes"] = {}
        for n in (2, 256, 4096):
            dev.set_probes(cloud[:n])            # warm: code object, buffers
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                cells = dev.set_probes(cloud[:n])
                ts.append(1e3 * (time.perf_counter() - t0))
            result["set_probes"][str(n)] = dict(summary(ts), found=int((cells >= 0).sum()))

        # ---- per call: A and B alternating
        dev.set_probes(np.array([a, b]))

        def host_path():
            x = dev.solution_owned               # nsx_get_solution: the whole vector
            return dofs.pressure_difference(x, a, b)[0]

        def device_path():
            p = dev.eval_probes()["pressure"]
            return float(p[0] - p[1])

        for _ in range(3):                       # warm both
            va, vb = host_path(), device_path()
        ta, tb = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            va = host_path()
            t1 = time.perf_counter()
            vb = device_path()
            t2 = time.perf_counter()
            ta.append(1e3 * (t1 - t0))
            tb.append(1e3 * (t2 - t1))
        sa, sb = summary(ta), summary(tb)
        diff = sa["median_ms"] - sb["median_ms"]
        noise = max(sa["spread_ms"], sb["spread_ms"])
        result["per_call"] = {"A_get_solution_plus_host_search": sa, "B_eval_probes": sb, "A_minus_B_median_ms": diff,
                              "largest_run_to_run_spread_ms": noise, "gain_exceeds_3x_spread": bool(diff > 3 * noise),
                              "ratio_A_over_B_medians": sa["median_ms"] / sb["median_ms"] if sb["median_ms"] > 0 else None,
                              "value_A": va, "value_B": vb, "abs_difference_of_the_values": abs(va - vb)}
        # ---- the two kernels by HIP events (launch scopes probe_locate / probe_eval), in a pass of its own
        dev.profile(True)
        dev.profile_reset()
        dev.set_probes(cloud)
        for _ in range(args.repeats):
            dev.eval_probes()
        tab = dev.profile_table()
        dev.profile(False)
        result["kernels"] = {k: {"us_per_launch": 1e3 * tab[k]["total_ms"] / tab[k]["launches"], "launches": tab[k]["launches"],
                                 "algorithmic_bytes_per_launch": tab[k]["bytes_per_launch"], "points": len(cloud)}
                             for k in ("probe_locate", "probe_eval") if k in tab and tab[k]["launches"]}
    finally:
        dev.close()
    text = json.dumps(result, indent=1)
    if args.out and args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"per_call": {k: result["per_call"][k] for k in ("A_minus_B_median_ms", "largest_run_to_run_spread_ms", "gain_exceeds_3x_spread", "ratio_A_over_B_medians")},
                      "A_median_ms": sa["median_ms"], "B_median_ms": sb["median_ms"],
                      "set_probes_median_ms": {k: v["median_ms"] for k, v in result["set_probes"].items()}, "kernels": result["kernels"]}))


if __name__ == "__main__":
    main()
