"""GPU suite: the tracer particles (include/nsx.h: nsx_set_tracers / nsx_advect_tracers / nsx_get_tracers; csrc/nsx_tracer.hip) against
closed-form pathlines and against the extended-precision restatement tests/tracer_reference.py (pinned by tests/test_tracer_reference.py).

Tolerance: positions within 1e-12 L, L the diagonal of the mesh's bounding box -- the project's standing 1e-12.  A substep adds a few dozen
roundings of relative size 1.1e-16 to a position of size <= L (lambda, ten shape functions, NP2 products per component, the stage sums), and
at most 32 substeps are taken: some 1e-14 L, two orders below the bound.  Discrete results (status, cell, exit face) are compared on the
particles whose decisions the reference took with a margin > 1e-9 in lambda ("sure").
Particle counts 1, 63, 64, 65 and 257 cross the edges of the 64-lane workgroups.  Measured maxima go to conftest.record (DESIGN.md section 5
quotes them).  Tests need a real MI355X."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import probe_reference as PR
import tracer_reference as TR
from conftest import Problem, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
COUNTS = (1, 63, 64, 65, 257)
KEYS = ("positions", "cells", "status", "exit_faces", "age")
_f64p, _i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2 if p.dim == 3 else 3), time)


def same_bits(a, b, n=None):
    return all(np.array_equal(a[k][:n], b[k][:n]) for k in KEYS)


def parity(name, test, got, ref, mesh):
    """positions of ALL particles within TOL * L; status, cell and exit face equal on the sure ones; returns the measured maximum / L"""
    L = TR.diagonal(mesh)
    err = float(np.abs(got["positions"].astype(np.longdouble) - ref["positions_ld"]).max() / L)
    found = ref["status"] != TR.NOT_FOUND
    sure = ref["margin"] > 1e-9
    age = float(np.abs(got["age"] - ref["age"]).max())
    print(name, "position error / L = %.2e, age error %.2e, unsure %d of %d, hops <= %d" % (err, age, (found & ~sure).sum(), found.sum(), ref["hops"].max()))
    record(test, case=name, position_over_L=err, age=age, unsure=int((found & ~sure).sum()), max_hops=int(ref["hops"].max()),
           active=int((ref["status"] == TR.ACTIVE).sum()), exited=int((ref["status"] == TR.EXITED).sum()), lost=int((ref["status"] == TR.LOST).sum()))
    assert err <= TOL, (name, err)
    for k in ("status", "cells", "exit_faces"):
        assert np.array_equal(got[k][sure], ref[k][sure]), (name, k)
    assert np.array_equal(got["status"] == TR.NOT_FOUND, ~found)
    assert age <= 1e-14 * max(1.0, float(np.abs(ref["age"]).max()))
    return err


# ---------------------------------------------------------------------------------------------- 1. closed forms
@pytest.mark.parametrize("kind,dim,n_cells", [("box", 2, 18), ("box", 3, 108), ("cube", 3, 6)])
def test_uniform_field_and_rigid_rotation_follow_the_closed_forms(kind, dim, n_cells):
    """box: 18 triangles / 108 tetrahedra; cube level 1: 6 cells.  Uniform field: x0 + u T whatever the scheme; rigid rotation u = A (x - c):
    P^n (x0 - c) + c with the scheme's polynomial P in hA (tests/tracer_reference.py: linear_closed_form)."""
    p = Problem(kind, dim, 1) if kind == "cube" else Problem(kind, dim)
    assert p.dofs.n_cells == n_cells
    V = np.asarray(p.mesh.vertices)
    lo, hi = V.min(axis=0), V.max(axis=0)
    c, L = (lo + hi) / 2, TR.diagonal(p.mesh)
    b = np.array([0.25, -0.5, 0.125][:dim]) * (hi - lo).min()
    A = TR.rotation_matrix(dim)
    pts = PR.box_points(p.mesh, 257, seed=9, shrink=0.5)
    start = PR.locate(p.mesh, pts)[0]
    n_sub = 8
    cases = [("uniform", TR.linear_state(p.dofs, np.zeros((dim, dim)), c, b), 0.4, s, None) for s in (TR.EULER, TR.RK4)]
    cases += [("rotation", TR.linear_state(p.dofs, A, c), dt, s, A) for s in (TR.EULER, TR.RK2, TR.RK4) for dt in (0.25, -0.25)]
    dev = p.device()
    worst = 0.0
    try:
        for name, state, dt, scheme, mat in cases:
            dev.set_solution(state)
            if mat is None:
                exact = pts.astype(np.longdouble) + np.longdouble(dt) * b
            else:
                exact = TR.linear_closed_form(pts, mat, c, np.longdouble(dt) / n_sub, n_sub, scheme)
            for n in COUNTS:
                status = dev.set_tracers(pts[:n])
                assert (status == TR.ACTIVE).all()
                dev.advect_tracers(dt, n_sub, scheme, TR.FROZEN)
                got = dev.get_tracers()
                assert (got["status"] == TR.ACTIVE).all() and (got["exit_faces"] == -1).all(), (name, scheme, n)
                err = float(np.abs(got["positions"].astype(np.longdouble) - exact[:n]).max() / L)
                worst = max(worst, err)
                assert err <= TOL, (name, scheme, dt, n, err)
                assert np.abs(got["age"] - dt).max() <= 1e-15
                if n == 257:
                    assert (got["cells"] != start).mean() > 0.1, (name, scheme)      # the walk was needed
                    again = PR.locate(p.mesh, got["positions"])
                    sure = again[3] > 1e-9
                    assert sure.mean() > 0.9 and np.array_equal(got["cells"][sure], again[0][sure])
        print("%s%dd: largest position error / L = %.2e" % (kind, dim, worst))
        record("tracers_closed_form", case="%s%dd" % (kind, dim), position_over_L=worst)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 2. parity on the cylinder
CYLINDER = {"3d-l1": (3, 1, 0.25, 16), "2d-l2": (2, 2, 0.5, 8), "3d-l1-backward": (3, 1, -0.25, 8)}
_cache = {}


def cylinder_case(name):
    """(problem, state, seeds, reference) of one cylinder case, computed once per session and never changed"""
    if name not in _cache:
        dim, level, dt, n_sub = CYLINDER[name]
        p = Problem("cylinder", dim, level)
        u = p.smooth_velocity()
        pts = PR.box_points(p.mesh, 200, seed=5)
        _cache[name] = (p, u, pts, TR.run(p.mesh, p.dofs, u, pts, dt, n_sub, TR.RK4))
    return _cache[name]


@pytest.mark.parametrize("name", list(CYLINDER))
def test_parity_with_the_reference_on_the_cylinder(name):
    dim, level, dt, n_sub = CYLINDER[name]
    p, u, pts, ref = cylinder_case(name)
    assert p.dofs.n_cells == (2832 if dim == 3 else 632)
    # against a vacuous pass, on the reference itself
    found = ref["status"] != TR.NOT_FOUND
    assert (~found).sum() == 1
    assert ((ref["margin"] <= 1e-9) & found).sum() <= 0.05 * found.sum()
    assert (ref["status"] == TR.EXITED).sum() >= 0.2 * found.sum() and (ref["status"] == TR.ACTIVE).sum() >= 0.5 * found.sum()
    dev = p.device()
    try:
        dev.set_solution(u)
        dev.set_tracers(pts)
        dev.advect_tracers(dt, n_sub, TR.RK4, TR.FROZEN)
        got = dev.get_tracers()
        parity("cylinder" + name, "tracers_parity", got, ref, p.mesh)
        lost = got["status"] == TR.NOT_FOUND
        assert np.array_equal(got["positions"][lost], pts[lost]) and (got["cells"][lost] == -1).all() and (got["age"][lost] == 0).all()
        assert (got["exit_faces"][got["status"] != TR.EXITED] == -1).all() and (got["exit_faces"][got["status"] == TR.EXITED] >= 0).all()
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 3. LINEAR field, read-only contract
def test_linear_field_spans_the_solved_step_and_the_call_reads_only():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("box", 2, n=[4, 3], hi=[1.0, 0.41])
    assert p.dofs.n_cells == 24
    pts = PR.box_points(p.mesh, 200, seed=5)
    dev, twin, fresh = p.device(), p.device(), p.device()
    try:
        for h in (dev, twin):
            h.set_solution(np.zeros(p.dofs.n_dofs))
            h.assemble(nsx.TEMAM)
            h.apply_boundary_values(*_bc(p, p.deltat))
        prev = dev.solution                                                          # what the solve copies into previous_solution
        for h in (dev, twin):
            h.solve_time_step(nsx.YOSIDA)
        sol = dev.solution
        assert np.array_equal(sol, twin.solution) and not np.array_equal(sol, prev)
        umax = float(np.abs(sol[:p.dofs.n_u]).max())
        assert np.isfinite(umax) and umax > 0
        T = 0.3 / umax                                                               # the fastest particle crosses a third of the box
        results = {}
        for dt in (T, -T):
            ref = TR.run(p.mesh, p.dofs, sol, pts, dt, 8, TR.RK4, TR.LINEAR, previous=prev)
            found = ref["status"] != TR.NOT_FOUND
            assert ((ref["margin"] <= 1e-9) & found).sum() <= 0.05 * found.sum() and ref["hops"].max() >= 1
            assert (ref["status"] == TR.ACTIVE).any()
            dev.set_tracers(pts)
            dev.advect_tracers(dt, 8, TR.RK4, TR.LINEAR)
            results[dt] = dev.get_tracers()
            parity("box2d-linear-%s" % ("forward" if dt > 0 else "backward"), "tracers_linear", results[dt], ref, p.mesh)
            frozen = TR.run(p.mesh, p.dofs, sol, pts, dt, 8, TR.RK4, TR.FROZEN)
            assert np.abs(frozen["positions_ld"] - ref["positions_ld"]).max() > 1e-6 * TR.diagonal(p.mesh)   # the field is not the frozen one
        # FROZEN reads `solution` alone: a handle whose previous_solution is still zero gives the same bits
        dev.set_tracers(pts)
        dev.advect_tracers(T, 8, TR.RK4, TR.FROZEN)
        a = dev.get_tracers()
        fresh.set_solution(dev.solution_owned)
        assert np.array_equal(fresh.solution, sol)
        fresh.set_tracers(pts)
        fresh.advect_tracers(T, 8, TR.RK4, TR.FROZEN)
        assert same_bits(a, fresh.get_tracers())
        # the calls changed no state: the next step is bitwise the twin's that never advected
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.rhs, twin.rhs)
        stats = []
        for h in (dev, twin):
            h.assemble_time_step(nsx.TEMAM)
            h.apply_boundary_values(*_bc(p, 2 * p.deltat))
            if h is dev:
                h.advect_tracers(T, 4, TR.RK2, TR.LINEAR)                             # between the boundary values and the solve
            stats.append(h.solve_time_step(nsx.YOSIDA))
        for key in ("outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "status", "final_residual"):
            assert stats[0][key] == stats[1][key], key
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.solution_owned, twin.solution_owned)
    finally:
        for h in (dev, twin, fresh):
            h.close()


# ---------------------------------------------------------------------------------------------- 4. bitwise properties
def test_prefixes_repeated_calls_and_two_runs_give_the_same_bits():
    p, u, pts, _ = cylinder_case("3d-l1")
    pts = np.concatenate([pts, PR.box_points(p.mesh, 57, seed=6)])
    assert len(pts) == 257
    dev = p.device()
    try:
        dev.set_solution(u)

        def go(n, calls, dt, n_sub):
            dev.set_tracers(pts[:n])
            for _ in range(calls):
                dev.advect_tracers(dt, n_sub, TR.RK4, TR.FROZEN)
            return dev.get_tracers()
        full = go(257, 1, 0.25, 16)
        assert (full["status"] == TR.EXITED).any() and (full["status"] == TR.ACTIVE).sum() > 100
        for n in (1, 63, 64, 65):
            assert same_bits(go(n, 1, 0.25, 16), full, n), n
        assert same_bits(go(257, 1, 0.25, 16), full)                                  # two identical runs
        twice = go(257, 2, 0.125, 8)                                                  # the same h, the same substeps: state and age persist
        assert same_bits(twice, full)
        active = full["status"] == TR.ACTIVE
        assert np.array_equal(full["age"][active], np.full(active.sum(), 0.25)) and (full["age"][~active] < 0.25).all()
        # finished particles never move again
        dev.advect_tracers(0.25, 4, TR.EULER, TR.FROZEN)
        later = dev.get_tracers()
        done = ~active
        assert same_bits({k: v[done] for k, v in later.items()}, {k: v[done] for k, v in twice.items()})
        assert dev.set_tracers(np.zeros((0, 3))).size == 0                            # n = 0 clears the set
        assert dev.L.nsx_get_tracers(dev._h, None, None, None, None, None) == -1
    finally:
        dev.close()


def test_layout_and_rank_tables_change_no_bit():
    """the three handles of tests/test_gpu_probes.py::test_layout_and_rank_tables_change_no_bit: the cell order, the cell-local node order and
    the geometry are the same on all three"""
    from navierstokes_project_nm4pde_amd import nsx
    p, u, pts, ref = cylinder_case("3d-l1")
    p4 = Problem("cylinder", 3, 1, n_sub=4)
    assert np.array_equal(p.mesh.cells, p4.mesh.cells) and np.array_equal(p.mesh.vertices, p4.mesh.vertices)
    u4 = np.zeros_like(u)
    u4[np.asarray(p4.dofs.cell_dofs).ravel()] = u[np.asarray(p.dofs.cell_dofs).ravel()]   # the same state, dof by dof
    results = []
    for name, make, state in (("plain", lambda: p.device(), u),
                              ("layout", lambda: nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(4, nsx.COLOUR, 0)), u),
                              ("ranks4", lambda: p4.device(), u4)):
        dev = make()
        try:
            dev.set_solution(state)
            dev.set_tracers(pts)
            dev.advect_tracers(0.25, 16, TR.RK4, TR.FROZEN)
            results.append((name, dev.get_tracers()))
            if name == "plain":
                # a layout and a rank table requested AFTER the set: it survives with its state (the vectors are reset: hand the state over)
                dev.set_tracers(pts)
                dev.advect_tracers(0.125, 8, TR.RK4, TR.FROZEN)
                dev.set_internal_layout(4, nsx.COLOUR, 0)
                assert dev.layout_info()["on"]
                dev.set_solution(state)
                dev.advect_tracers(0.125, 8, TR.RK4, TR.FROZEN)
                results.append(("layout-after", dev.get_tracers()))
        finally:
            dev.close()
    parity("cylinder3d-l1-plain", "tracers_layout", results[0][1], ref, p.mesh)
    for name, got in results[1:]:
        assert same_bits(got, results[0][1]), name


# ---------------------------------------------------------------------------------------------- 5. errors and lifetime
def test_a_nan_in_the_state_loses_the_particles_that_meet_it_and_the_call_returns():
    p, u, pts, _ = cylinder_case("2d-l2")
    bad = u.copy()
    X = np.asarray(p.dofs.support_points)
    bad[:p.dofs.n_u][X[:p.dofs.n_u, 0] > 1.1] = float("nan")                         # the downstream half of the channel
    ref = TR.run(p.mesh, p.dofs, bad, pts, 0.5, 8, TR.RK4)
    assert (ref["status"] == TR.LOST).sum() > 20 and (ref["status"] == TR.ACTIVE).sum() > 20
    dev = p.device()
    try:
        dev.set_solution(bad)
        dev.set_tracers(pts)
        assert dev.L.nsx_advect_tracers(dev._h, 0.5, 8, TR.RK4, TR.FROZEN) == 0       # NSX_OK
        got = dev.get_tracers()
        parity("cylinder2d-l2-nan", "tracers_nan", got, ref, p.mesh)
        lost = got["status"] == TR.LOST
        assert np.isfinite(got["positions"]).all() and (got["exit_faces"][lost] == -1).all() and (got["cells"][lost] >= 0).all()
    finally:
        dev.close()


def test_argument_errors_and_lifetime():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    pts = np.ascontiguousarray(PR.pressure_points(2))
    pp = pts.ctypes.data_as(_f64p)
    dev = p.device()
    try:
        L, h = dev.L, dev._h
        dev.set_solution(p.smooth_velocity())
        assert L.nsx_advect_tracers(h, 0.1, 1, TR.RK4, TR.FROZEN) == -1               # no set yet
        assert L.nsx_get_tracers(h, None, None, None, None, None) == -1
        assert L.nsx_set_tracers(h, -1, pp, -1.0) == -1
        assert L.nsx_set_tracers(h, 2, None, -1.0) == -1
        assert L.nsx_set_tracers(h, 2, pp, 1.0) == -1 and L.nsx_set_tracers(h, 2, pp, float("nan")) == -1
        for value in (float("nan"), float("inf")):
            seeds = pts.copy()
            seeds[1, 0] = value
            assert L.nsx_set_tracers(h, 2, seeds.ctypes.data_as(_f64p), -1.0) == -1
        many = np.zeros((1048577, 2))
        assert L.nsx_set_tracers(h, 1048577, many.ctypes.data_as(_f64p), -1.0) == -3
        assert b"1048576" in L.nsx_last_error(h)
        assert L.nsx_set_tracers(None, 2, pp, -1.0) == -1
        assert L.nsx_get_tracers(h, None, None, None, None, None) == -1               # none of the refused calls left a set behind
        for tol in (0.0, 0.5, -1.0, -7.0):
            assert L.nsx_set_tracers(h, 2, pp, tol) == 0
        assert L.nsx_advect_tracers(h, float("nan"), 1, TR.RK4, TR.FROZEN) == -1 and L.nsx_advect_tracers(h, float("inf"), 1, TR.RK4, TR.FROZEN) == -1
        assert L.nsx_advect_tracers(h, 0.1, 0, TR.RK4, TR.FROZEN) == -1 and L.nsx_advect_tracers(h, 0.1, -3, TR.RK4, TR.FROZEN) == -1
        assert L.nsx_advect_tracers(h, 0.1, 1, 3, TR.FROZEN) == -1 and L.nsx_advect_tracers(h, 0.1, 1, 0, TR.FROZEN) == -1
        assert L.nsx_advect_tracers(h, 0.1, 1, TR.RK4, 2) == -1 and L.nsx_advect_tracers(h, 0.1, 1, TR.RK4, -1) == -1
        status, age = np.empty(2, np.int32), np.empty(2)
        assert L.nsx_get_tracers(h, None, None, status.ctypes.data_as(_i32p), None, age.ctypes.data_as(_f64p)) == 0   # any output may be NULL
        assert status.tolist() == [TR.ACTIVE, TR.ACTIVE] and age.tolist() == [0.0, 0.0]   # the refused calls moved nothing
        assert L.nsx_advect_tracers(h, 0.01, 2, TR.RK4, TR.LINEAR) == 0                # previous_solution is zero before the first solve: allowed
        # the tracer set and the probe set are independent of each other
        assert dev.set_tracers(pts).tolist() == [TR.ACTIVE, TR.ACTIVE]
        dev.set_probes(PR.box_points(p.mesh, 5))
        assert dev.get_tracers()["status"].tolist() == [TR.ACTIVE, TR.ACTIVE] and len(dev.eval_probes()["pressure"]) == 5
        dev.set_tracers(np.zeros((0, 2)))
        assert len(dev.eval_probes()["pressure"]) == 5
        assert L.nsx_set_tracers(h, 2, pp, -1.0) == 0
        # a second nsx_set_mesh drops the set
        cd = np.ascontiguousarray(p.dofs.cell_dofs, dtype=np.int32)
        cc = np.ascontiguousarray(p.dofs.cell_coords, dtype=np.float64)
        assert L.nsx_set_mesh(h, p.dofs.n_cells, p.dofs.dofs_per_cell, cd.ctypes.data_as(_i32p), cc.ctypes.data_as(_f64p), p.dofs.n_u, p.dofs.n_p) == 0
        assert L.nsx_get_tracers(h, None, None, None, None, None) == -1 and L.nsx_advect_tracers(h, 0.1, 1, TR.RK4, TR.FROZEN) == -1
        assert b"nsx_set_tracers" in L.nsx_last_error(h)
        assert L.nsx_set_tracers(h, 2, pp, -1.0) == 0 and L.nsx_get_tracers(h, None, None, None, None, None) == 0
        # a non-manifold mesh is refused: the first cell handed over twice makes three cells around each of its faces' neighbours
        dup = np.concatenate([cd, cd[:1]])
        ccd = np.concatenate([cc, cc[:1]])
        if L.nsx_set_mesh(h, len(dup), p.dofs.dofs_per_cell, dup.ctypes.data_as(_i32p), ccd.ctypes.data_as(_f64p), p.dofs.n_u, p.dofs.n_p) == 0:
            assert L.nsx_set_tracers(h, 2, pp, -1.0) == -1 and b"more than two cells" in L.nsx_last_error(h)
            assert L.nsx_get_tracers(h, None, None, None, None, None) == -1
    finally:
        dev.close()
    # handles without a mesh (raw calls, as tests/test_abi.py makes them)
    L = nsx.lib()
    h = ctypes.c_void_p()
    prm = nsx.Params(2, 0, 1e-3, 1e-2)
    assert L.nsx_create(ctypes.byref(prm), ctypes.byref(h)) == 0
    try:
        assert L.nsx_set_tracers(h, 2, pp, -1.0) == -1                               # neither tables nor mesh
        t = p.tables
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.N2, t.dN2, t.N1, t.weights)]
        # a (dim, n_p2) other than (2, 6) / (3, 10) never gets as far as a mesh: nsx_set_tables refuses it with NSX_ERR_UNSUPPORTED
        assert L.nsx_set_tables(h, t.n_q, 10, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == -3
        assert L.nsx_set_tables(h, t.n_q, t.n_p2, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == 0
        assert L.nsx_set_tracers(h, 2, pp, -1.0) == -1 and b"nsx_set_mesh" in L.nsx_last_error(h)   # tables, no mesh
        assert L.nsx_advect_tracers(h, 0.1, 1, TR.RK4, TR.FROZEN) == -1 and L.nsx_get_tracers(h, None, None, None, None, None) == -1
    finally:
        L.nsx_destroy(h)


def test_a_one_rank_communicator_works_and_no_call_issues_a_collective():
    p = Problem("cylinder", 2, 1)
    single, plain = p.device(), p.device()
    try:
        single.set_solution(p.smooth_velocity())
        single.comm_init_single()
        before = single.comm_counters()
        seeds = PR.box_points(p.mesh, 65, seed=5)
        single.set_tracers(seeds)
        single.advect_tracers(0.1, 4, TR.RK4, TR.FROZEN)
        got = single.get_tracers()
        assert single.comm_counters() == before
        assert (got["status"] == TR.ACTIVE).sum() > 30
        plain.set_solution(p.smooth_velocity())
        plain.set_tracers(seeds)
        plain.advect_tracers(0.1, 4, TR.RK4, TR.FROZEN)
        assert same_bits(got, plain.get_tracers())
    finally:
        single.close()
        plain.close()


def test_distributed_handles_refuse_tracers_without_a_collective(tmp_path):
    """2D cylinder level 1 on 2 processes (one card, gloo, host callbacks), the launch recipe of
    tests/test_gpu_probes.py::test_distributed_probes_have_one_owner_and_every_rank_the_same_values on a master port of its own"""
    world = 2
    prefix = str(tmp_path / "tracers")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29603", os.path.join(ROOT, "tests", "tracers_dist_worker.py"), "2", "1", prefix]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(world):
        d = json.load(open("%s_rank%d.json" % (prefix, k)))
        assert d["world"] == world and d["rank"] == k
        assert d["rc"] == {"set": -3, "advect": -3, "get": -3}, d
        assert "processes" in d["message"]
        assert d["before"] == d["after"]                                             # neither an all-reduce nor a ghost exchange
        assert d["probes_found"] > 0                                                 # the handle itself works


# ---------------------------------------------------------------------------------------------- 6. executable
def test_executable_writes_the_tracer_series_only_when_asked(tmp_path):
    """navier_stokes2D level:1 3 4 with NSX_TRACERS=5 appends five rows per step to tracers_2D.csv; its last rows are what the three calls
    give behind the same three steps driven from Python (the recipe of tests/test_gpu_probes.py's executable test)."""
    import re
    import __graft_entry__ as ge
    ge.build()
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    dim, n = 2, 5
    exe = os.path.join(ROOT, "navierstokes_project_nm4pde_amd", "host", "navier_stokes%dD" % dim)
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    env = {k: v for k, v in os.environ.items() if k != "NSX_TRACERS"}
    out = subprocess.run([exe, "level:1", "3", "4"], cwd=with_dir, env=dict(env, NSX_TRACERS=str(n)), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain = subprocess.run([exe, "level:1", "3", "4"], cwd=without_dir, env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    assert not (without_dir / "tracers_2D.csv").exists()

    def untimed(text):
        return [line for line in text.splitlines() if not re.search(r"[Tt]ime taken|seconds|elapsed", line)]
    assert untimed(out.stdout) == untimed(plain.stdout) and len(untimed(out.stdout)) > 10
    rows = np.loadtxt(with_dir / "tracers_2D.csv", delimiter=",")
    assert rows.shape == (3 * n, 9)                                                  # step, time, particle, x, y, cell, status, exit face, age
    assert rows[:, 0].astype(int).tolist() == [1] * n + [2] * n + [3] * n and rows[:, 2].astype(int).tolist() == list(range(n)) * 3
    assert (rows[:, 6] == TR.ACTIVE).all() and np.allclose(rows[:, 8], rows[:, 1], rtol=0, atol=1e-15)   # age = time while ACTIVE
    mesh = Mesh.cylinder(dim, 1).partition(1, 4)
    dofs, tables = DoFs(mesh, "colour"), Tables(dim)
    dt = 0.01
    seeds = np.stack([np.full(n, 0.1), 0.1 + 0.2 * np.arange(n) / (n - 1)], axis=1)
    dev = nsx.Nsx(dofs, tables, 1e-3, dt)
    try:
        dev.set_solution(np.zeros(dofs.n_dofs))
        assert (dev.set_tracers(seeds) == TR.ACTIVE).all()
        inlet = InletVelocity(dim, 2)
        t = 0.0
        for step in range(3):
            t += dt
            if step == 0:
                dev.assemble(nsx.TEMAM)
            else:
                dev.assemble_time_step(nsx.TEMAM)
            dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, t))
            dev.solve_time_step(3, inner_maxiter=10000)
            dev.advect_tracers(dt, 4, TR.RK4, TR.LINEAR)
        got = dev.get_tracers()
    finally:
        dev.close()
    last = rows[2 * n:]
    assert np.abs(last[:, 3:5] - got["positions"]).max() <= TOL * TR.diagonal(mesh)
    assert np.abs(got["positions"] - seeds).max() > 1e-4                            # they moved
    assert np.array_equal(last[:, 5].astype(int), got["cells"]) and np.array_equal(last[:, 7].astype(int), got["exit_faces"])
