#!/usr/bin/env python3
"""What one Q-criterion isosurface costs on the problem bench.py times (the 1 089 643-DoF 3D cylinder as bench.py builds it: first-touch
numbering on one rank, 4096 virtual ranks laid out inside libnsx, Yosida, reference tolerances), behind a few solved steps so that `solution`
is that of a run -- against what a user does for it without the extraction:

  A  "volume"   nsx_get_nodal_field(NSX_FIELD_Q): the download of one value per P2 node, the host contouring that has to follow NOT counted
  B  "surface"  nsx_extract_isosurface(NSX_ISO_NODAL Q at the isovalue, coloured by the speed) + nsx_get_isosurface (points, colour, cells)

Both follow one nsx_compute_nodal_fields, whose time is measured beside them and belongs to both.  A and B alternate in one process, wall
times with the stream synchronised inside the calls; the alternation runs twice and the difference of a variant's medians between the two
rounds is the run-to-run difference.  A gain is claimed only at three times that difference (the project's standing rule).  The per-kernel
times of B come from the launch scopes (nsx_profile_get) of separate profiled calls.  Everything goes to profiles/iso_extract_<level>.json.

    python tools/iso_timing.py [--steps 3] [--pairs 15] [--level 7] [--ranks 4096] [--quantile 0.98] [--out profiles/iso_extract_l7.json]
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
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="time steps solved before the measurement")
    ap.add_argument("--pairs", type=int, default=15, help="A/B pairs per round (two rounds)")
    ap.add_argument("--level", type=int, default=bench.BASE_LEVEL)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--quantile", type=float, default=0.98, help="the isovalue is this quantile of the nodal Q")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.numbering, args.ordering, args.schur_blocks = "first_touch", "colour", 0   # bench.py's defaults
    out_path = args.out or os.path.join(ROOT, "profiles", "iso_extract_l%d.json" % args.level)

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
            dev.solve_time_step(nsx.YOSIDA)
        dev.compute_nodal_fields()
        q = dev.nodal_field(nsx.FIELD_Q)[:, 0]
        iso = float(np.quantile(q, args.quantile))
        field, colour = nsx.iso_source(nsx.ISO_NODAL, which=nsx.FIELD_Q), nsx.iso_source(nsx.ISO_VELOCITY, component=-1)
        t0 = time.perf_counter()
        pts, col, cells = dev.extract_isosurface(field, iso, colour)        # uploads the coordinates and builds the node maps
        first_ms = 1e3 * (time.perf_counter() - t0)
        result = {"dofs": int(dofs.n_dofs), "cells": int(dofs.n_cells), "p2_nodes": int(dofs.n_u // 3), "level": args.level, "virtual_ranks": args.ranks,
                  "steps_solved": args.steps, "q_quantile": args.quantile, "isovalue": iso, "n_primitives": int(len(cells)),
                  "active_cells": int(len(np.unique(cells))), "first_extract_with_uploads_ms": first_ms,
                  "volume_bytes": int(q.nbytes), "surface_bytes": int(pts.nbytes + col.nbytes + cells.nbytes), "all_finite": bool(np.isfinite(pts).all())}

        def timed(f):
            t = time.perf_counter()
            f()
            return 1e6 * (time.perf_counter() - t)
        variants = {"compute_nodal_fields": dev.compute_nodal_fields, "A_volume_download": lambda: dev.nodal_field(nsx.FIELD_Q),
                    "B_surface_extract_and_get": lambda: dev.extract_isosurface(field, iso, colour)}
        rounds = []
        for _ in range(2):
            t = {k: [] for k in variants}
            for _ in range(args.pairs):
                for k, f in variants.items():                             # A and B alternate
                    t[k].append(timed(f))
            rounds.append({k: summary(v) for k, v in t.items()})
        result["rounds"] = rounds
        med = {k: statistics.median([r[k]["median_us"] for r in rounds]) for k in variants}
        r2r = {k: abs(rounds[0][k]["median_us"] - rounds[1][k]["median_us"]) for k in variants}
        result["median_us"], result["run_to_run_us"] = med, r2r
        gain = med["A_volume_download"] - med["B_surface_extract_and_get"]
        noise = max(r2r["A_volume_download"], r2r["B_surface_extract_and_get"])
        result["B_faster_than_A_by_us"] = gain
        result["gain_claimed"] = bool(gain >= 3.0 * noise and gain > 0)
        # the kernels of B, between HIP events
        kernels = {}
        for _ in range(args.pairs):
            dev.profile(True)
            dev.profile_reset()
            dev.extract_isosurface(field, iso, colour)
            tab = dev.profile_table()
            dev.profile(False)
            for name, e in tab.items():
                if name.startswith("iso_"):
                    kernels.setdefault(name, {"us": [], "bytes": e["bytes_per_launch"]})["us"].append(1e3 * e["total_ms"] / e["launches"])
        result["kernels"] = {k: dict(summary(v["us"]), algorithmic_bytes_per_launch=v["bytes"],
                                     bytes_per_s_at_median=v["bytes"] / (1e-6 * statistics.median(v["us"]))) for k, v in kernels.items()}
    finally:
        dev.close()
    text = json.dumps(result, indent=1)
    if out_path != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"n_primitives": result["n_primitives"], "median_us": med, "run_to_run_us": r2r, "gain_claimed": result["gain_claimed"],
                      "kernels_median_us": {k: v["median_us"] for k, v in result["kernels"].items()}}))


if __name__ == "__main__":
    main()
