#!/usr/bin/env python3
"""What a 256^3 lattice of velocity and pressure costs on the problem bench.py times (the 1 089 643-DoF 3D cylinder as bench.py builds it:
first-touch numbering on one rank, 4096 virtual ranks laid out inside libnsx, Yosida, reference tolerances), behind a few solved steps so that
`solution` is that of a run -- against the only route there was before the lattice sampling:

  A  "probes"   one nsx_set_probes + nsx_eval_probes per chunk of 65536 points (256 chunks for 256^3): a few chunks, spread over the
                lattice, are timed and the total is EXTRAPOLATED as (mean over the chunks) * (number of chunks)
  B  "lattice"  nsx_set_lattice (once per lattice) and nsx_eval_lattice(velocity | pressure) (per step), and the download nsx_get_lattice

The lattice spans the bounding box of the mesh.  Wall times with the stream synchronised inside the calls.  Every B call is repeated; the
repetitions run in two rounds and the difference of a variant's medians between the two rounds is the run-to-run difference.  The
per-kernel times of B come from the launch scopes (nsx_profile_get) of separate profiled calls.  No ratio is promised anywhere: the figures
go to profiles/lattice_<level>_<n>.json and from there into DESIGN.md section 5.

    python tools/lattice_timing.py [--steps 3] [--n 256] [--reps 5] [--chunks 3] [--level 7] [--ranks 4096] [--out profiles/lattice_l7_256.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 65536


def summary(v):
    v = sorted(float(x) for x in v)
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="time steps solved before the measurement")
    ap.add_argument("--n", type=int, default=256, help="lattice points per axis")
    ap.add_argument("--reps", type=int, default=5, help="repetitions of every lattice call per round (two rounds)")
    ap.add_argument("--chunks", type=int, default=3, help="probe chunks of 65536 points that are timed")
    ap.add_argument("--level", type=int, default=bench.BASE_LEVEL)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.numbering, args.ordering, args.schur_blocks = "first_touch", "colour", 0   # bench.py's defaults
    out_path = args.out or os.path.join(ROOT, "profiles", "lattice_l%d_%d.json" % (args.level, args.n))

    import numpy as np
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh, dofs, tables = bench.build_problem(args.level, args.ranks, numbering="first_touch", ranks_input=1)
    V = np.asarray(mesh.vertices, dtype=np.float64)
    counts = np.array([args.n] * 3, dtype=np.int32)
    origin, spacing = V.min(axis=0), (V.max(axis=0) - V.min(axis=0)) / (args.n - 1)
    n_total = int(np.prod(counts.astype(np.int64)))
    what = nsx.LATTICE_VELOCITY | nsx.LATTICE_PRESSURE
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

        def timed(f):
            t = time.perf_counter()
            r = f()
            return 1e6 * (time.perf_counter() - t), r
        first_us, n_found = timed(lambda: dev.set_lattice(origin, spacing, counts))   # uploads the vertex coordinates of the cells
        result = {"dofs": int(dofs.n_dofs), "cells": int(dofs.n_cells), "level": args.level, "virtual_ranks": args.ranks, "steps_solved": args.steps,
                  "counts": [int(c) for c in counts], "n_total": n_total, "n_found": int(n_found), "first_set_lattice_with_upload_us": first_us}
        variants = {"B_set_lattice": lambda: dev.set_lattice(origin, spacing, counts), "B_eval_lattice_u_p": lambda: dev.eval_lattice(what),
                    "B_get_lattice_u": lambda: dev.get_lattice(nsx.LATTICE_VELOCITY)}
        rounds = []
        for _ in range(2):
            t = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, f in variants.items():
                    t[k].append(timed(f)[0])
            rounds.append({k: summary(v) for k, v in t.items()})
        result["rounds"] = rounds
        med = {k: statistics.median([r[k]["median_us"] for r in rounds]) for k in variants}
        r2r = {k: abs(rounds[0][k]["median_us"] - rounds[1][k]["median_us"]) for k in variants}
        cells = dev.lattice_cells().ravel()
        # A: a few chunks of the same points through the probes, spread over the lattice (first, middle, last, ...)
        n_chunks = (n_total + CHUNK - 1) // CHUNK
        picks = sorted(set(int(round(k * (n_chunks - 1) / max(args.chunks - 1, 1))) for k in range(args.chunks)))
        ax = [origin[d] + np.arange(args.n, dtype=np.float64) * spacing[d] for d in range(3)]
        set_us, eval_us, agree = [], [], True
        for c in picks:
            lin = np.arange(c * CHUNK, min((c + 1) * CHUNK, n_total), dtype=np.int64)
            pts = np.stack([ax[0][lin % args.n], ax[1][lin // args.n % args.n], ax[2][lin // (args.n * args.n)]], axis=1)
            us, found = timed(lambda: dev.set_probes(pts))
            set_us.append(us)
            eval_us.append(timed(lambda: dev.eval_probes())[0])
            agree = agree and bool(np.array_equal(found, cells[lin]))
        dev.set_probes(np.zeros((0, 3)))
        result["A_probe_chunks"] = {"chunk_points": CHUNK, "chunks_in_lattice": n_chunks, "chunks_timed": picks, "set_probes_us": set_us, "eval_probes_us": eval_us,
                                    "owners_agree_with_lattice": agree}
        med["A_set_probes_extrapolated"] = statistics.mean(set_us) * n_chunks
        med["A_eval_probes_extrapolated"] = statistics.mean(eval_us) * n_chunks
        r2r["A_set_probes_extrapolated"] = (max(set_us) - min(set_us)) * n_chunks
        r2r["A_eval_probes_extrapolated"] = (max(eval_us) - min(eval_us)) * n_chunks
        result["median_us"], result["run_to_run_us"] = med, r2r
        # the kernels of B, between HIP events
        kernels = {}
        for _ in range(args.reps):
            dev.profile(True)
            dev.profile_reset()
            dev.set_lattice(origin, spacing, counts)
            dev.eval_lattice(what)
            tab = dev.profile_table()
            dev.profile(False)
            for name, e in tab.items():
                if name.startswith("lattice_"):
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
    print(json.dumps({"n_total": n_total, "n_found": result["n_found"], "median_us": med, "run_to_run_us": r2r,
                      "owners_agree": result["A_probe_chunks"]["owners_agree_with_lattice"],
                      "kernels_median_us": {k: v["median_us"] for k, v in result["kernels"].items()}}))


if __name__ == "__main__":
    main()
