#!/usr/bin/env python3
"""A/B of the inner precision (include/nsx.h: nsx_set_inner_precision) on the problem bench.py times: the 1 089 643-DoF 3D cylinder
as bench.py builds it (deal.II's first-touch numbering on one rank, 4096 virtual ranks laid out inside libnsx, Schur blocks of <= 96
rows, u0 = 0 with the inlet switched on impulsively, Yosida, reference tolerances, the reference's schedule of the preconditioner set-up).

After the first step, the spin-up and the warm-up the steps ALTERNATE FP64 / FP32 step by step in ONE process, on one handle -- the two
precisions see the same state of the flow, the same clocks and the same neighbours on the card:

  pass 1 (no event pairs in the launch stream): per step t_prec, t_solve, outer and inner-F iterations -> ms per outer iteration
  pass 2 (nsx_profile_enable): per step the per-launch time and the algorithmic bytes of the inner F product scopes (spmv_F, spmv_F_if)
         and of the velocity triangular-solve scope (ilu_solve_F) -> mean and spread over the steps, float / double ratios

    python tools/inner_precision_ab.py [--steps 20] [--warmup 5] [--spinup 20] [--level 7] [--ranks 4096] [--out profiles/inner_fp32_kernels.json]

The scope "spmv_F" also holds the ONE double product per step of the right-hand side (mass matrix times the previous solution, in
assembly): the FP32 row is a mean over ~690 float launches and that one double launch (below 0.1 % of the figure; the profiler's
per-kernel rows separate them).

Kernel times are confirmed by a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats -- python tools/inner_precision_ab.py --steps 4 --spinup 4 --out /dev/null
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCOPES = ("spmv_F", "spmv_F_if", "ilu_solve_F", "F_to_f32", "ilu_factor_F", "mgs_sweep", "spmv_saddle_u")


def mean_spread(v):
    v = [float(x) for x in v]
    if not v:
        return None
    return {"mean": statistics.fmean(v), "min": min(v), "max": max(v), "stdev": statistics.pstdev(v) if len(v) > 1 else 0.0, "n": len(v)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed steps PER PRECISION in each of the two passes")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spinup", type=int, default=20)
    ap.add_argument("--level", type=int, default=bench.BASE_LEVEL)
    ap.add_argument("--ranks", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inner_fp32_kernels.json"))
    args = ap.parse_args()
    args.numbering, args.ordering, args.schur_blocks = "first_touch", "colour", 0   # bench.py's defaults

    import numpy as np
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh, dofs, tables = bench.build_problem(args.level, args.ranks, numbering="first_touch", ranks_input=1)
    cache_env = os.environ.get("NSX_SCHUR_CACHE")
    if cache_env is None:
        os.environ["NSX_SCHUR_CACHE"] = "0"   # the reference's schedule, as bench.py's headline
    dev = nsx.Nsx(dofs, tables, bench.NU, bench.DT, layout=bench.layout_of(args, dofs), inner_precision=nsx.INNER_FP64)
    try:
        inlet = InletVelocity(3)
        dev.set_solution(np.zeros(dofs.n_dofs))
        t = [0.0]

        def one_step(first=False, precision=None):
            t[0] += bench.DT
            if precision is not None:
                dev.set_inner_precision(precision)
            if first:
                dev.assemble(nsx.TEMAM)
            else:
                dev.assemble_time_step(0)
            dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, t[0]))
            return dev.solve_time_step(nsx.YOSIDA)

        one_step(True)
        for k in range(args.spinup + args.warmup):
            one_step(precision=(nsx.INNER_FP64, nsx.INNER_FP32)[k % 2])   # both precisions warm (buffers of the float streams allocated)
        names = {nsx.INNER_FP64: "fp64", nsx.INNER_FP32: "fp32"}
        result = {"dofs": int(dofs.n_dofs), "level": args.level, "virtual_ranks": args.ranks, "steps_per_precision": args.steps,
                  "spinup": args.spinup, "warmup": args.warmup, "schur_cache": os.environ.get("NSX_SCHUR_CACHE") != "0"}
        # ---- pass 1: step times
        rows = {"fp64": [], "fp32": []}
        for k in range(2 * args.steps):
            prec = (nsx.INNER_FP64, nsx.INNER_FP32)[k % 2]
            st = one_step(precision=prec)
            info = dev.path_info()
            rows[names[prec]].append({"outer": st["outer_iterations"], "inner_F": st["inner_F_iterations"], "inner_S": st["inner_S_iterations"],
                                      "t_prec_ms": 1e3 * st["t_prec"], "t_solve_ms": 1e3 * st["t_solve"], "F_float": info["inner_F_fp32"], "ilu_float": info["ilu_F_fp32"]})
        result["steps"] = {}
        for name, r in rows.items():
            result["steps"][name] = {
                "ms_per_outer_iteration": mean_spread([x["t_solve_ms"] / max(1, x["outer"]) for x in r]),
                "ms_per_outer_iteration_pooled": sum(x["t_solve_ms"] for x in r) / max(1, sum(x["outer"] for x in r)),
                "t_prec_ms": mean_spread([x["t_prec_ms"] for x in r]), "t_solve_ms": mean_spread([x["t_solve_ms"] for x in r]),
                "outer": mean_spread([x["outer"] for x in r]), "inner_F": mean_spread([x["inner_F"] for x in r]),
                "inner_F_per_outer": sum(x["inner_F"] for x in r) / max(1, sum(x["outer"] for x in r)),
                "float_streams": [max(x["F_float"] for x in r), max(x["ilu_float"] for x in r)], "per_step": r}
        # ---- pass 2: per-launch times and algorithmic bytes
        dev.profile(True)
        per = {"fp64": {}, "fp32": {}}
        for k in range(2 * args.steps):
            prec = (nsx.INNER_FP64, nsx.INNER_FP32)[k % 2]
            dev.profile_reset()
            one_step(precision=prec)
            tab = dev.profile_table()
            for sc in SCOPES:
                e = tab.get(sc)
                if e and e["launches"] > 0:
                    d = per[names[prec]].setdefault(sc, {"us": [], "bytes": [], "launches": []})
                    d["us"].append(1e3 * e["total_ms"] / e["launches"])
                    d["bytes"].append(e["bytes_per_launch"])
                    d["launches"].append(e["launches"])
        dev.profile(False)
        result["kernels"] = {}
        for name in per:
            result["kernels"][name] = {}
            for sc, d in per[name].items():
                us, b = mean_spread(d["us"]), statistics.fmean(d["bytes"])
                result["kernels"][name][sc] = {"us_per_launch": us, "algorithmic_bytes_per_launch": b, "launches_per_step": statistics.fmean(d["launches"]),
                                               "fraction_of_hbm_peak": b / (us["mean"] * 1e-6) / (bench.HBM_PEAK_GBS * 1e9) if us["mean"] > 0 else None}
        result["ratio_fp32_over_fp64"] = {}
        for sc in ("spmv_F", "spmv_F_if", "ilu_solve_F"):
            a, b = result["kernels"]["fp64"].get(sc), result["kernels"]["fp32"].get(sc)
            if a and b:
                result["ratio_fp32_over_fp64"][sc] = {"time": b["us_per_launch"]["mean"] / a["us_per_launch"]["mean"],
                                                      "algorithmic_bytes": b["algorithmic_bytes_per_launch"] / a["algorithmic_bytes_per_launch"]}
        s64, s32 = result["steps"]["fp64"], result["steps"]["fp32"]
        result["ratio_fp32_over_fp64"]["ms_per_outer_iteration"] = s32["ms_per_outer_iteration_pooled"] / s64["ms_per_outer_iteration_pooled"]
        result["paths"] = dev.path_info()
        result["layout"] = dev.layout_info()
    finally:
        dev.close()
        if cache_env is None:
            os.environ.pop("NSX_SCHUR_CACHE", None)
    text = json.dumps(result, indent=1)
    if args.out and args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    brief = {"ratio_fp32_over_fp64": result["ratio_fp32_over_fp64"],
             "ms_per_outer_iteration": {k: result["steps"][k]["ms_per_outer_iteration_pooled"] for k in result["steps"]},
             "us_per_launch": {k: {sc: v["us_per_launch"]["mean"] for sc, v in result["kernels"][k].items()} for k in result["kernels"]}}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
