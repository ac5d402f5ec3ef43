"""The seams of a time step: the vector operations around the inner solves folded into neighbouring launches (NSX_STEP_FUSED).  It is the
same computation as the statement-by-statement sequence: every comparison here is BITWISE -- np.array_equal on solutions, equal outer /
inner-F / inner-S counts, final_residual ==.

The switch is read by the library per call, so two handles fed identically run under different settings inside one process.  Meshes: the suite's smallest cylinders (3D level 1, 2D level 2)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import Problem

pytestmark = pytest.mark.gpu

SERIAL = {"NSX_STEP_FUSED": "0"}
PRECS = {"yosida": 0, "simple": 1, "ayosida": 2, "asimple": 3}  # nsx.YOSIDA, SIMPLE, AYOSIDA, ASIMPLE
TOLS = {"reference": (1e-4, 1e-2), "parity": (1e-11, 1e-10)}
MESHES = {"3d-l1": (3, 1), "2d-l2": (2, 2)}
COUNTS = ("status", "outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "final_residual", "persistent_fallbacks")


@contextmanager
def env(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_problems = {}


def problem(mesh, n_sub=1):
    key = (mesh, n_sub)
    if key not in _problems:
        dim, level = MESHES[mesh]
        _problems[key] = Problem("cylinder", dim, level, n_sub=n_sub, ordering="colour" if n_sub > 1 else "first_touch")
    return _problems[key]


def bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2 if p.dim == 3 else 3), time)


def make(mesh, layout):
    """(problem, handle) of one of the layouts: plain (one rank: the workgroup-per-block / levelled triangular solves, seconds per
    solve), internal layout (8, colour, 96), a rank table with 4 ranks, the same table under a 1-rank communicator"""
    import navierstokes_project_nm4pde_amd.nsx as nsx
    p = problem(mesh, 4 if layout in ("ranks", "comm") else 1)
    dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, nsx.COLOUR, 96) if layout == "internal" else None)
    if layout == "comm":
        dev.comm_init_single()
    return p, dev


@pytest.fixture(scope="module")
def pairs():
    """two handles per (mesh, layout), created once: every test feeds both the same state first"""
    made = {}

    def get(mesh, layout):
        if (mesh, layout) not in made:
            p, a = make(mesh, layout)
            _, b = make(mesh, layout)
            made[(mesh, layout)] = (p, a, b)
        return made[(mesh, layout)]

    yield get
    for _, a, b in made.values():
        a.close()
        b.close()


def feed(dev, p, step, u0=None):
    """state and system of time step `step` (0-based); step 0 starts from u0"""
    import navierstokes_project_nm4pde_amd.nsx as nsx
    if step == 0:
        dev.set_solution(u0)
        dev.assemble(nsx.TEMAM)
    else:
        dev.assemble_time_step(0)
    dev.apply_boundary_values(*bc(p, (step + 1) * p.deltat))


def same_step(sa, sb, xa, xb, what):
    for k in COUNTS:
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])
    assert np.array_equal(xa, xb), (what, float(np.abs(xa - xb).max()))


def run_steps(p, a, b, env_a, env_b, prec, tol, inner, what, n_steps=3, inner_maxiter=100000):
    u0 = p.smooth_velocity()
    out = []
    for step in range(n_steps):
        res = []
        for dev, e in ((a, env_a), (b, env_b)):
            feed(dev, p, step, u0)
            with env(e):
                st = dev.solve_time_step(prec, tol_abs=tol, inner_rtol=inner, inner_maxiter=inner_maxiter, check=False)
            res.append((st, dev.solution_owned.copy()))
        same_step(res[0][0], res[1][0], res[0][1], res[1][1], (what, step))
        out.append(res[0][0])
    return out


@pytest.mark.parametrize("layout", ["plain", "internal", "ranks", "comm"])
@pytest.mark.parametrize("tol", list(TOLS))
@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("mesh", list(MESHES))
def test_whole_steps_fused_against_serial(pairs, mesh, prec, tol, layout):
    """three time steps on two handles fed identically, one on the statement-by-statement sequence, compared after every step"""
    p, a, b = pairs(mesh, layout)
    stats = run_steps(p, a, b, {}, SERIAL, PRECS[prec], *TOLS[tol], (mesh, prec, tol, layout))
    assert all(s["status"] == 0 and s["outer_iterations"] > 0 for s in stats)
    assert a.persistent_state()["fallbacks"] == 0 and b.persistent_state()["fallbacks"] == 0


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("mesh", list(MESHES))
def test_prec_vmult_with_the_switch_off_and_on(pairs, mesh, prec):
    """nsx_prec_vmult on ONE handle, NSX_STEP_FUSED switched between the calls: random src, the same dst going in (aSIMPLE reads it)"""
    p, a, _ = pairs(mesh, "ranks")
    feed(a, p, 0, p.smooth_velocity())
    a.prec_initialize(PRECS[prec])
    rng = np.random.default_rng(7)
    src, dst0 = rng.standard_normal(p.dofs.n_dofs), rng.standard_normal(p.dofs.n_dofs)
    res = []
    for flag in ("0", "1", "0", "1"):
        with env({"NSX_STEP_FUSED": flag}):
            res.append(a.prec_vmult(PRECS[prec], src, inner_rtol=1e-6, dst0=dst0))
    for x, st in res[1:]:
        assert np.array_equal(res[0][0], x), (prec, float(np.abs(res[0][0] - x).max()))
        for k in ("inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "status"):
            assert st[k] == res[0][1][k], (prec, k)
    assert np.isfinite(res[0][0]).all() and res[0][1]["status"] == 0


# An inner velocity solve that needs more than the 28 iterations of a GMRES cycle: the cycles after the first start from x != 0 and
# take the existing k_axpy_multi, the first the variants that do not read x.  Block-Jacobi ILU(0) on these small meshes converges in a
# handful of iterations at any tolerance above the rounding level of the residual, so the rank table is the finest the mesh allows
# sensibly (many small blocks: a weak preconditioner) and the inner tolerance sits just above that level.
# Measured on the serial handle (Yosida, outer tolerance 1e-9), inner-F iterations per solve: 2D level 2 with 16 ranks 18.6 / 21.9 / 23.8 /
# 27.8 at 1e-10 / 1e-12 / 1e-13 / 1e-14 -- no tolerance reaches 28 there; 3D level 1 with 8 ranks 24.0 / 28.5 / 31.2 / 33.4.
RESTART = {"mesh": "3d-l1", "n_sub": 8, "inner_rtol": 1e-14, "inner_maxiter": 400}


@pytest.mark.parametrize("prec", ["yosida", "asimple"])
def test_restart_cycle_inside_an_inner_velocity_solve(prec):
    import navierstokes_project_nm4pde_amd.nsx as nsx
    p = problem(RESTART["mesh"], RESTART["n_sub"])
    a = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat)
    b = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat)
    try:
        stats = run_steps(p, a, b, SERIAL, {}, PRECS[prec], 1e-9, RESTART["inner_rtol"], ("restart", prec), n_steps=1, inner_maxiter=RESTART["inner_maxiter"])
        s = stats[0]  # the serial handle's
        print("restart cycles: %d inner-F iterations in %d solves, %d outer, status %d" % (s["inner_F_iterations"], s["n_F_solves"], s["outer_iterations"], s["status"]))
        # the precondition of this test: on average more than one cycle per solve, so cycles with x != 0 have run
        assert s["inner_F_iterations"] > 28 * s["n_F_solves"], (s["inner_F_iterations"], s["n_F_solves"])
    finally:
        a.close()
        b.close()


def test_fused_launches_are_the_ones_that_run(pairs):
    """The event profiler's table of one Yosida step with NSX_STEP_FUSED=0 and =1: per application of the preconditioner (one Schur solve
    each) the fused sequence has three k_axpby launches fewer -- tmp -= src_p, the residual of the first velocity solve's cycle and
    dst_u = -dst_u + res -- and the same products, reductions, triangular solves and basis updates.  (Exact while every inner solve takes
    one cycle, which the reference's inner tolerance gives on this mesh; copies and fills have no scope of their own.)"""
    p, a, b = pairs("3d-l1", "ranks")
    tables = []
    for dev, flag in ((a, "0"), (b, "1")):
        feed(dev, p, 0, p.smooth_velocity())
        dev.profile(True)
        dev.profile_reset()
        with env({"NSX_STEP_FUSED": flag}):
            st = dev.solve_time_step(0, tol_abs=1e-4, inner_rtol=1e-2)
        tables.append(({k: v["launches"] for k, v in dev.profile_table().items() if v["launches"] > 0}, st, dev.solution_owned.copy()))
        dev.profile(False)
    (t0, s0, x0), (t1, s1, x1) = tables
    same_step(s0, s1, x0, x1, "profiled")
    n = s0["n_S_solves"]
    print("launches per scope, unfused / fused:", {k: (t0.get(k, 0), t1.get(k, 0)) for k in sorted(set(t0) | set(t1))}, "applications:", n)
    assert n > 0 and s0["n_F_solves"] == 2 * n
    assert t0["axpby"] - t1["axpby"] == 3 * n, (t0["axpby"], t1["axpby"], n)
    for scope in ("dot", "axpy_multi", "spmv_F", "spmv_B", "spmv_G", "ilu_solve_F"):
        assert t0[scope] == t1[scope], (scope, t0[scope], t1[scope])
