"""bench.py without a GPU: the committed evidence every bench line quotes is where bench.py looks for it and says what the
code says (a kernel renamed without regenerating profiles/, a moved profile, a changed strong_10M schedule would otherwise
only show up as nulls in a driver's record)."""
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    import importlib
    return importlib.import_module("bench")


def test_committed_profiles_are_where_bench_reads_them():
    b = _bench()
    for rel in (b.PMC_PROFILE, b.LAYOUT_PROFILE, b.BIG_BASE_PROFILE, b.STEP_HISTORY):
        assert os.path.isfile(os.path.join(ROOT, rel)), rel
    base = b.committed_big_base()
    assert base and base["n_dofs"] == b.BIG_DOFS and base["value"] > 0 and base["ms_per_outer_iteration"] > 0
    # the one-GPU base was measured with the schedule the N > 1 leg uses
    assert (base["steps"], base["warmup"], base["spinup_steps"]) == (b.BIG_STEPS, b.BIG_WARMUP, b.BIG_SPINUP)
    mean = b.long_run_mean_outer()
    assert mean and 15.0 < mean < 60.0
    lay = b.committed_layouts()
    assert lay and lay["rows"]


def test_kernels_named_in_bench_exist_in_the_committed_profiles():
    b = _bench()
    with open(os.path.join(ROOT, b.PMC_PROFILE)) as f:
        pmc = json.load(f)
    with open(os.path.join(ROOT, "profiles", "r05_kernel_stats_bench_steps5.csv")) as f:
        stats = [r["Name"] for r in csv.DictReader(f)]
    for scope in ("spmv_F", "ilu_solve_F", "mgs_sweep", "cg_S"):
        name = b.KERNEL_OF[scope]
        assert name in pmc, (scope, name)
        assert any(s.startswith(name + "(") for s in stats), (scope, name)
        t, src = b.pmc_traffic(scope)
        assert t and t > 1e6 and src == b.PMC_PROFILE, (scope, t, src)


def test_committed_bench_line_carries_the_contract_fields():
    with open(os.path.join(ROOT, "profiles", "r05_bench.json")) as f:
        d = json.loads(f.read().strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "time-steps/s" and d["dtype"] == "f64" and d["n_gpus"] == 1 and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["traffic"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["cpu_model"] and "march=native" in c["compiler_flags"]
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    # since round 5 `value` is like for like (the Schur product, ILU(S) and the block inverses rebuilt in every step as the reference does,
    # Preconditioners.hpp:358-362); the hoisted figure of rounds 1-4 stands beside it, measured on the same steps
    assert d["schur_cache"] is False and d["value_hoisted"] > d["value"] and d["hoisted"]["same_iteration_history"] is True
    assert d["paths"]["spmv_lds_staged"] == 1 and d["paths"]["schur_cg_path"] == 2 and d["paths"]["fused_launches"] == 0


def test_bench_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--steps" in r.stdout and "--warmup" in r.stdout
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _args(*argv):
    """bench.py's options as main() sees them after its defaults are applied (one GPU)"""
    import argparse
    b = _bench()
    a = argparse.Namespace(full=False, cpu_only=False, layout_table=None, no_cpu=False, no_big=False, pmc="auto", level=None, comm="auto",
                           profile_steps=5)
    for k in argv:
        k, _, v = k.partition("=")
        setattr(a, k, v if v else True)
    return b, a


def test_a_plain_run_measures_the_headline_only():
    b, a = _args()
    assert b.extras(a, 1) == {"cpu_baseline": False, "pmc_live": False, "hoisted_twin": False, "profile_steps": 0, "self_p2p": False, "strong_10M": False}
    assert not any(b.extras(a, 4).values())
    b, a = _args("comm=rccl1")
    assert not any(b.extras(a, 1).values())


def test_full_measures_what_the_line_carries_beside_the_headline():
    b, a = _args("full")
    assert b.extras(a, 1) == {"cpu_baseline": True, "pmc_live": True, "hoisted_twin": True, "profile_steps": 5, "self_p2p": False, "strong_10M": False}
    assert b.extras(a, 4) == {"cpu_baseline": False, "pmc_live": False, "hoisted_twin": False, "profile_steps": 5, "self_p2p": False, "strong_10M": True}
    b, a = _args("full", "comm=rccl1", "no_cpu")
    e = b.extras(a, 1)
    assert e["self_p2p"] and not e["cpu_baseline"] and not e["pmc_live"]
    b, a = _args("cpu_only")  # the explicit CPU mode runs its leg with or without --full
    assert b.extras(a, 1)["cpu_baseline"] and b.extras(a, 1)["profile_steps"] == 0


def test_dump_outputs_writes_the_solution_in_float64(tmp_path):
    import numpy as np
    b = _bench()
    x = np.random.default_rng(7).standard_normal(1000)
    b.dump_outputs(str(tmp_path / "full"), 700, x)
    u, p = np.load(tmp_path / "full" / "velocity.npy"), np.load(tmp_path / "full" / "pressure.npy")
    assert u.dtype == np.float64 and p.dtype == np.float64 and (u == x[:700]).all() and (p == x[700:]).all()
    # above the limit: the same seeded sample in every run, within the limit
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), 700, x, limit=4000)
    u1, p1 = np.load(tmp_path / "s1" / "velocity.npy"), np.load(tmp_path / "s1" / "pressure.npy")
    assert u1.nbytes + p1.nbytes <= 4000 and len(u1) == 350 and len(p1) == 150
    assert (u1 == np.load(tmp_path / "s2" / "velocity.npy")).all() and (p1 == np.load(tmp_path / "s2" / "pressure.npy")).all()
    assert np.isin(u1, x[:700]).all() and np.isin(p1, x[700:]).all()
    assert b.DUMP_LIMIT_BYTES + 2 * 128 <= 64 * 10 ** 6


def test_round_tools_parse():
    """the measurement scripts the profiles were made with are at least valid bash / python (they run on the GPU box only)"""
    import glob
    import py_compile
    for sh in glob.glob(os.path.join(ROOT, "tools", "*.sh")):
        r = subprocess.run(["bash", "-n", sh], capture_output=True, text=True)
        assert r.returncode == 0, (sh, r.stderr)
    for py in glob.glob(os.path.join(ROOT, "tools", "*.py")):
        py_compile.compile(py, doraise=True)
