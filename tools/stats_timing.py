#!/usr/bin/env python3
"""What one nsx_stats_accumulate (velocity + pressure, one bin) costs on the problem bench.py times (the 1 089 643-DoF 3D cylinder as bench.py
builds it: first-touch numbering on one rank, 4096 virtual ranks laid out inside libnsx, so the update kernel reads the state through the
permutation), behind a few solved steps so that `solution` is that of a run -- against the device-to-device copy rate measured in the same
run and against the download of the state, the only route to running statistics there was before.

  kernel    k_stats_update between HIP events (the launch scope "stats_update", nsx_profile_get): warm, `reps` launches per round, two
            rounds; the difference of the rounds' means is the run-to-run difference.  Bytes: the algorithmic bytes the scope records
            (every operand once).
  copy      hipMemcpyAsync device to device (torch) of a buffer of HALF those bytes -- it reads and writes that many, the same traffic --
            between HIP events, warm, alternating with the kernel's rounds.
  --bins 8  eight bins fed round-robin and eight copy buffer pairs used round-robin: 0.5 GB of planes (and of copy buffers) between two
            uses of a line, so neither finds anything in the 256-MiB Infinity Cache -- the case of a run, where a solve lies between two
            accumulates.  With one bin both work out of that cache.
  --plain   a handle without an internal layout: the kernel reads the state directly instead of through the permutation.
  fraction  (kernel bytes / kernel time) / (copy traffic / copy time)
  wall      host clock around `reps` accumulates and one closing nsx_stats_get (the accumulates are enqueued, the get synchronises)
  download  host clock around nsx_get_solution (synchronises inside)

No ratio is promised anywhere: the figures go to profiles/stats_<level>.json and from there into DESIGN.md section 5.

    python tools/stats_timing.py [--steps 3] [--reps 200] [--level 7] [--ranks 4096] [--bins 1] [--plain] [--out profiles/stats_l7.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="time steps solved before the measurement")
    ap.add_argument("--reps", type=int, default=200, help="launches per round (two rounds)")
    ap.add_argument("--level", type=int, default=bench.BASE_LEVEL)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--bins", type=int, default=1, help="phase bins, fed round-robin (and as many copy buffer pairs): 8 keeps nothing in the Infinity Cache")
    ap.add_argument("--plain", action="store_true", help="no internal layout (the kernel reads the state without the permutation); no steps, a seeded state")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.numbering, args.ordering, args.schur_blocks = "first_touch", "colour", 0   # bench.py's defaults
    if args.plain:
        args.steps = 0
    out_path = args.out or os.path.join(ROOT, "profiles", "stats_l%d%s%s.json" % (args.level, "_plain" if args.plain else "", "_bins%d" % args.bins if args.bins > 1 else ""))

    import numpy as np
    import torch
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh, dofs, tables = bench.build_problem(args.level, args.ranks, numbering="first_touch", ranks_input=1)
    what = nsx.STATS_VELOCITY | nsx.STATS_PRESSURE
    dev = nsx.Nsx(dofs, tables, bench.NU, bench.DT, layout=None if args.plain else bench.layout_of(args, dofs))
    try:
        dev.set_solution(np.random.default_rng(1).standard_normal(dofs.n_dofs) if args.plain else np.zeros(dofs.n_dofs))
        inlet = InletVelocity(3)
        for step in range(args.steps):
            if step == 0:
                dev.assemble(nsx.TEMAM)
            else:
                dev.assemble_time_step(nsx.TEMAM)
            dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, (step + 1) * bench.DT))
            dev.solve_time_step(nsx.YOSIDA)
        dev.stats_begin(what, args.bins)
        for k in range(20 * args.bins):                          # warm: code object, first touch of the planes
            dev.stats_accumulate(k % args.bins, bench.DT)
        dev.stats_get(nsx.STATS_TKE, 0)

        def kernel_round():
            dev.profile(True)
            dev.profile_reset()
            for k in range(args.reps):
                dev.stats_accumulate(k % args.bins, bench.DT)
            dev.stats_get(nsx.STATS_TKE, 0)                      # synchronises
            e = dev.profile_table()["stats_update"]
            dev.profile(False)
            assert e["launches"] == args.reps
            return 1e3 * e["total_ms"] / e["launches"], e["bytes_per_launch"]

        us0, nbytes = kernel_round()
        half = int(nbytes) // 2 // 8 * 8
        pairs = [(torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")) for _ in range(args.bins)]

        def copy_round():
            for k in range(10 * args.bins):
                pairs[k % args.bins][1].copy_(pairs[k % args.bins][0])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.reps):
                pairs[k % args.bins][1].copy_(pairs[k % args.bins][0])
            b.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b) / args.reps

        kernel_us, copy_us = [], []
        for _ in range(2):                                       # alternating
            copy_us.append(copy_round())
            kernel_us.append(kernel_round()[0])

        def wall_round():
            t = time.perf_counter()
            for k in range(args.reps):
                dev.stats_accumulate(k % args.bins, bench.DT)
            dev.stats_get(nsx.STATS_TKE, 0)
            return 1e6 * (time.perf_counter() - t) / args.reps
        wall_us = [wall_round() for _ in range(2)]
        down_us = []
        for _ in range(7):
            t = time.perf_counter()
            dev.solution_owned
            down_us.append(1e6 * (time.perf_counter() - t))
        get_us = []
        for _ in range(5):
            t = time.perf_counter()
            dev.stats_get(nsx.STATS_STRESS_U, 0)
            get_us.append(1e6 * (time.perf_counter() - t))
        k, c = statistics.mean(kernel_us), statistics.mean(copy_us)
        result = {"dofs": int(dofs.n_dofs), "p2_nodes": int(dofs.n_u // 3), "p1_nodes": int(dofs.n_p), "level": args.level, "virtual_ranks": args.ranks,
                  "steps_solved": args.steps, "bins": args.bins, "internal_layout": not args.plain, "reps_per_round": args.reps, "first_round_kernel_us": us0,
                  "kernel_us_rounds": kernel_us, "kernel_us": k, "kernel_run_to_run_us": abs(kernel_us[0] - kernel_us[1]),
                  "algorithmic_bytes_per_launch": nbytes, "kernel_bytes_per_s": nbytes / (1e-6 * k),
                  "copy_buffer_bytes": half, "copy_us_rounds": copy_us, "copy_us": c, "copy_traffic_bytes_per_s": 2.0 * half / (1e-6 * c),
                  "fraction_of_copy_rate": (nbytes / k) / (2.0 * half / c),
                  "wall_us_per_accumulate_rounds": wall_us, "state_download_us_median": statistics.median(down_us),
                  "state_download_us_min_max": [min(down_us), max(down_us)], "stats_get_stress_us_median": statistics.median(get_us)}
    finally:
        dev.close()
    text = json.dumps(result, indent=1)
    if out_path != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: result[k] for k in ("kernel_us", "kernel_run_to_run_us", "algorithmic_bytes_per_launch", "kernel_bytes_per_s", "copy_us",
                                             "copy_traffic_bytes_per_s", "fraction_of_copy_rate", "wall_us_per_accumulate_rounds",
                                             "state_download_us_median")}))


if __name__ == "__main__":
    main()
