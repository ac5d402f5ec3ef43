"""GPU suite: the point probes (include/nsx.h: nsx_set_probes / nsx_get_probe_cells / nsx_eval_probes; csrc/nsx_probe.hip) against closed
forms and against the extended-precision restatement tests/probe_reference.py (itself pinned by tests/test_probe_reference.py).

Tolerance: |delta u_i| <= 1e-12 S_u,i, |delta p| <= 1e-12 S_p, |delta d_j u_i| <= 1e-12 S_g,ij with the absolute-term sums of the helper
(S_u = sum |N_a| |U_a|, S_p = sum |lambda_v| |P_v|, S_g = sum |U_a| |grad N_a|): the project's standing 1e-12 (tolerance (a) of
tests/test_gpu_diagnostics.py), scaled by the sum of the absolute terms so that it holds under cancellation.
The point tile of k_probe_locate is 64: the point counts 1, 2, 63, 64, 65 and 257 cross its edges.
Measured maxima go to conftest.record (DESIGN.md section 5 quotes them).  Tests need a real MI355X."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diagnostics_reference as R
import probe_reference as PR
from conftest import Problem, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
_f64p, _i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2 if p.dim == 3 else 3), time)


def recipe(p, n_uniform=200, n_support=200):
    """the points of the parity tests: uniform in the bounding box, P2 support points (ties), the two pressure points, three points outside
    the box and one in the cylinder's hole; returns (points, slices by name)"""
    parts = [("uniform", PR.box_points(p.mesh, n_uniform)), ("support", PR.support_points(p.dofs, n_support)),
             ("pressure", PR.pressure_points(p.dim)), ("outside", PR.outside_points(p.dim))]
    where, s = {}, 0
    for name, x in parts:
        where[name] = slice(s, s + len(x))
        s += len(x)
    return np.concatenate([x for _, x in parts]), where


def ratios(got, ref, grad_mask=None):
    """largest |delta| / S of velocity, pressure and gradient over the probes (0 / 0 = 0: where S vanishes the value has to be exactly 0)"""
    def q(d, s, mask=None):
        d, s = np.abs(d), np.asarray(s)
        if mask is not None:
            d, s = d[mask], s[mask]
        if d.size == 0:
            return 0.0
        r = np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d == 0, 0.0, np.inf))
        return float(np.max(r))
    m = {"u": q(got["velocity"] - ref["velocity"], ref["S_u"]), "p": q(got["pressure"] - ref["pressure"], ref["S_p"])}
    if "gradient" in got:
        m["grad"] = q(got["gradient"] - ref["gradient"], ref["S_g"], grad_mask)
    return m


def check(name, test, got, ref, grad_mask=None):
    m = ratios(got, ref, grad_mask)
    print(name, {k: "%.2e" % v for k, v in m.items()})
    record(test, case=name, **m)
    for k, v in m.items():
        assert v <= TOL, (name, k, v)
    return m


# ---------------------------------------------------------------------------------------------- 1. closed form
@pytest.mark.parametrize("kind,dim", [("box", 2), ("box", 3), ("cube", 3)])
def test_quadratic_velocity_and_linear_pressure_give_the_polynomials(kind, dim):
    """box: 18 triangles / 108 tetrahedra (one full 64-lane workgroup and a partial one); cube level 1: fewer cells than one wave"""
    p = Problem(kind, dim, 1) if kind == "cube" else Problem(kind, dim)
    assert p.dofs.n_cells == ({2: 18, 3: 108}[dim] if kind == "box" else 6)
    state = PR.quadratic_state(p.dofs)
    pts = PR.box_points(p.mesh, 65, shrink=0.02)                       # interior points
    ref = PR.evaluate(p.mesh, p.dofs, state, pts)
    u, G = R.quadratic_field(pts.astype(np.longdouble))
    exact = dict(ref, velocity=u.astype(np.float64), gradient=G.astype(np.float64), pressure=7.0 + pts @ np.array([2.0, -1.0, 0.5][:dim]))
    dev = p.device()
    try:
        dev.set_solution(state)
        cells = dev.set_probes(pts)
        got = dev.eval_probes(gradient=True)
        assert got["found"].all() and ref["found"].all()
        sure = (ref["mult"] == 1) & (ref["lam_min"] > 1e-9)
        assert sure.sum() > 50 and np.array_equal(cells[sure], ref["cells"][sure])
        check("%s%dd" % (kind, dim), "probes_closed_form", got, exact)
        check("%s%dd-helper" % (kind, dim), "probes_closed_form_helper", got, ref, grad_mask=ref["mult"] == 1)
        c2, owners, lam = dev.probe_cells()
        assert np.array_equal(c2, cells) and (owners == 0).all()
        assert np.abs(lam[sure] - ref["lam"][sure]).max() <= 1e-13 and np.abs(lam.sum(axis=1) - 1).max() <= 2e-15
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 2. parity with the helper
@pytest.mark.parametrize("dim,level", [(3, 1), (2, 2)])
def test_parity_with_the_helper(dim, level):
    p = Problem("cylinder", dim, level)
    assert p.dofs.n_cells == (2832 if dim == 3 else 632)
    u = p.smooth_velocity()
    pts, w = recipe(p)
    ref = PR.evaluate(p.mesh, p.dofs, u, pts)
    dev = p.device()
    try:
        dev.set_solution(u)
        cells = dev.set_probes(pts)
        got = dev.eval_probes(gradient=True)
        assert np.array_equal(got["found"], ref["found"])
        assert np.array_equal(cells >= 0, ref["found"])
        sure = (ref["mult"] == 1) & (ref["lam_min"] > 1e-9)
        assert np.array_equal(cells[sure], ref["cells"][sure])
        assert np.array_equal(cells[w["support"]], ref["cells"][w["support"]])      # ties: the lowest cell
        assert (ref["mult"][w["support"]] > 1).mean() > 0.5                          # (a mid-point of a boundary edge has one cell)
        # against a vacuous pass
        assert got["found"][w["uniform"]].mean() >= 0.9
        assert got["found"][w["support"]].all() and len(pts[w["support"]]) == 200
        assert got["found"][w["pressure"]].all()
        assert not got["found"][w["outside"]].any()
        for k in ("velocity", "pressure", "gradient"):
            assert not got[k][~got["found"]].any()                                   # exact zeros
        check("cylinder%dd-l%d" % (dim, level), "probes_parity", got, ref, grad_mask=ref["mult"] == 1)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 3. tile edges
def test_every_prefix_of_the_point_list_gives_the_same_bits():
    p = Problem("box", 3)
    state = PR.quadratic_state(p.dofs)
    pts = np.concatenate([PR.box_points(p.mesh, 200), PR.support_points(p.dofs, 57)])
    order = np.random.default_rng(3).permutation(len(pts))
    pts = pts[order]
    assert len(pts) == 257
    dev = p.device()
    try:
        dev.set_solution(state)
        full_cells = dev.set_probes(pts)
        full = dev.eval_probes(gradient=True)
        _, full_owners, full_lam = dev.probe_cells()
        assert full["found"].all()
        for n in (1, 2, 63, 64, 65, 257):
            cells = dev.set_probes(pts[:n])
            _, owners, lam = dev.probe_cells()
            got = dev.eval_probes(gradient=True)
            assert np.array_equal(cells, full_cells[:n]) and np.array_equal(owners, full_owners[:n]) and np.array_equal(lam, full_lam[:n]), n
            for k in ("velocity", "pressure", "gradient", "found"):
                assert np.array_equal(got[k], full[k][:n]), (n, k)
        assert len(dev.set_probes(np.zeros((0, 3)))) == 0                            # n_points = 0 clears the set
        assert dev.L.nsx_eval_probes(dev._h, None, None, None, None) == -1
        assert dev.L.nsx_get_probe_cells(dev._h, None, None, None) == -1
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 4. layout invariance
def test_layout_and_rank_tables_change_no_bit():
    """the three handles of tests/test_gpu_diagnostics.py::test_layout_and_rank_tables_change_no_bit.  The cell order, the cell-local node
    order and the geometry are the same on all three, so the same cell, the same lambda and the same nodal values meet in the same
    arithmetic: every bit is the same, for the 4-rank numbering as well."""
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 3, 1)
    p4 = Problem("cylinder", 3, 1, n_sub=4)
    assert np.array_equal(p.mesh.cells, p4.mesh.cells) and np.array_equal(p.mesh.vertices, p4.mesh.vertices)
    u = p.smooth_velocity()
    u4 = np.zeros_like(u)
    u4[np.asarray(p4.dofs.cell_dofs).ravel()] = u[np.asarray(p.dofs.cell_dofs).ravel()]   # the same state, dof by dof
    pts, _ = recipe(p, 100, 100)
    ref = PR.evaluate(p.mesh, p.dofs, u, pts)
    results = []
    for name, make, state in (("plain", lambda: p.device(), u),
                              ("layout", lambda: nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, nsx.COLOUR, 0)), u),
                              ("ranks4", lambda: p4.device(), u4)):
        dev = make()
        try:
            dev.set_solution(state)
            dev.set_probes(pts)
            results.append((name, dev.probe_cells(), dev.eval_probes(gradient=True)))
            if name == "layout":
                assert dev.layout_info()["on"] and dev.layout_info()["ranks"] == 8
            if name == "plain":
                # a layout requested AFTER the probes: the set survives (the state vectors are reset: hand the state over again)
                dev.set_internal_layout(8, nsx.COLOUR, 0)
                assert dev.layout_info()["on"]
                dev.set_solution(state)
                results.append(("layout-after", dev.probe_cells(), dev.eval_probes(gradient=True)))
        finally:
            dev.close()
    _, pc_ref, ev_ref = results[0]
    assert ev_ref["found"].sum() > 190
    check("cylinder3d-l1-plain", "probes_layout", ev_ref, ref, grad_mask=ref["mult"] == 1)
    for name, pc, ev in results[1:]:
        for a, b in zip(pc, pc_ref):
            assert np.array_equal(a, b), name
        check("cylinder3d-l1-" + name, "probes_layout", ev, ref, grad_mask=ref["mult"] == 1)
        for k in ("velocity", "pressure", "gradient", "found"):
            assert np.array_equal(ev[k], ev_ref[k]), (name, k)


# ---------------------------------------------------------------------------------------------- 5. purity and reproducibility
def test_the_call_changes_no_state_and_two_calls_agree_bitwise():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    u = p.smooth_velocity()
    a, b = PR.pressure_points(2)
    pts = np.concatenate([PR.pressure_points(2), PR.box_points(p.mesh, 30)])
    dev, twin = p.device(), p.device()
    try:
        for h in (dev, twin):
            h.set_solution(u)
        dev.set_probes(pts)
        e0 = dev.eval_probes(gradient=True)                                          # before the assembly
        for h in (dev, twin):
            h.assemble(nsx.TEMAM)
            h.apply_boundary_values(*_bc(p, p.deltat))
        e1 = dev.eval_probes(gradient=True)                                          # between the boundary values and the solve
        e2 = dev.eval_probes(gradient=True)
        for k in e1:
            assert np.array_equal(e1[k], e2[k]), k
        assert not np.array_equal(e0["velocity"], e1["velocity"])                    # the Dirichlet values are in `solution` now
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.rhs, twin.rhs)
        sa = dev.solve_time_step(nsx.YOSIDA)
        sb = twin.solve_time_step(nsx.YOSIDA)
        for key in ("outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "status"):
            assert sa[key] == sb[key], key
        assert sa["final_residual"] == sb["final_residual"]
        e3 = dev.eval_probes(gradient=True)                                          # after the solve
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.solution_owned, twin.solution_owned)
        assert np.array_equal(dev.rhs, twin.rhs)
        sol = dev.solution
        ref = PR.evaluate(p.mesh, p.dofs, sol, pts)
        check("cylinder2d-l1-solved", "probes_after_solve", e3, ref, grad_mask=ref["mult"] == 1)
        front, n_found = p.dofs.pressure_difference(sol, a, b)
        assert n_found == 2 and e3["found"][:2].all()
        err = abs((e3["pressure"][0] - e3["pressure"][1]) - front)
        record("probes_pressure_difference", case="cylinder2d-l1", err=err, bound=TOL * (ref["S_p"][0] + ref["S_p"][1]), value=front)
        assert err <= TOL * (ref["S_p"][0] + ref["S_p"][1])
    finally:
        dev.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 6. not finite
def test_a_nan_shows_up_in_exactly_the_probes_whose_cell_holds_it():
    p = Problem("cylinder", 3, 1)
    cd = np.asarray(p.dofs.cell_dofs)
    u = p.smooth_velocity()
    dof = int(cd[p.dofs.n_cells // 2, 1])                                             # second velocity component of a vertex
    assert dof < p.dofs.n_u
    u[dof] = float("nan")
    holders = np.flatnonzero((cd == dof).any(axis=1))
    centroids = np.asarray(p.dofs.cell_coords)[holders].mean(axis=1)                 # a probe inside every cell that holds the dof
    pts = np.concatenate([recipe(p)[0], centroids])
    dev = p.device()
    try:
        dev.set_solution(u)
        cells = dev.set_probes(pts)
        vel, pres, grad = np.empty((len(pts), 3)), np.empty(len(pts)), np.empty((len(pts), 3, 3))
        found = np.empty(len(pts), np.int32)
        rc = dev.L.nsx_eval_probes(dev._h, vel.ctypes.data_as(_f64p), pres.ctypes.data_as(_f64p), grad.ctypes.data_as(_f64p), found.ctypes.data_as(_i32p))
        assert rc == 0                                                               # the values propagate, the call succeeds
        holds = np.zeros(len(pts), dtype=bool)
        holds[cells >= 0] = (cd[cells[cells >= 0]] == dof).any(axis=1)
        assert len(holders) <= holds.sum() < len(pts) and np.array_equal(cells[-len(holders):], holders)
        assert np.array_equal(~np.isfinite(vel).all(axis=1), holds)
        assert np.array_equal(~np.isfinite(grad).all(axis=(1, 2)), holds)
        assert np.isnan(vel[holds, 1]).all() and np.isfinite(vel[:, [0, 2]]).all() and np.isfinite(pres).all()
        # a point coordinate that is not finite is an argument error
        bad = pts[:3].copy()
        bad[1, 2] = float("nan")
        assert dev.L.nsx_set_probes(dev._h, 3, bad.ctypes.data_as(_f64p), -1.0) == -1
        bad[1, 2] = float("inf")
        assert dev.L.nsx_set_probes(dev._h, 3, bad.ctypes.data_as(_f64p), -1.0) == -1
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    pts = np.ascontiguousarray(PR.pressure_points(2))
    pp = pts.ctypes.data_as(_f64p)
    dev = p.device()
    try:
        L, h = dev.L, dev._h
        assert L.nsx_eval_probes(h, None, None, None, None) == -1                    # no probe set yet
        assert L.nsx_get_probe_cells(h, None, None, None) == -1
        assert L.nsx_set_probes(h, -1, pp, -1.0) == -1
        assert L.nsx_set_probes(h, 2, None, -1.0) == -1
        assert L.nsx_set_probes(h, 2, pp, 1.0) == -1 and L.nsx_set_probes(h, 2, pp, 2.0) == -1
        assert L.nsx_set_probes(h, 2, pp, float("nan")) == -1
        many = np.zeros((65537, 2))
        assert L.nsx_set_probes(h, 65537, many.ctypes.data_as(_f64p), -1.0) == -3
        assert b"65536" in L.nsx_last_error(h)
        assert L.nsx_set_probes(None, 2, pp, -1.0) == -1
        assert L.nsx_eval_probes(h, None, None, None, None) == -1                    # none of the refused calls left a set behind
        for tol in (0.0, 0.5, -1.0, -7.0):
            assert L.nsx_set_probes(h, 2, pp, tol) == 0
        pres, found = np.empty(2), np.empty(2, np.int32)
        assert L.nsx_eval_probes(h, None, pres.ctypes.data_as(_f64p), None, found.ctypes.data_as(_i32p)) == 0   # any output may be NULL
        assert found.tolist() == [1, 1]
        assert L.nsx_get_probe_cells(h, None, None, None) == 0
        # a second nsx_set_mesh drops the set
        cd = np.ascontiguousarray(p.dofs.cell_dofs, dtype=np.int32)
        cc = np.ascontiguousarray(p.dofs.cell_coords, dtype=np.float64)
        assert L.nsx_set_mesh(h, p.dofs.n_cells, p.dofs.dofs_per_cell, cd.ctypes.data_as(_i32p), cc.ctypes.data_as(_f64p), p.dofs.n_u, p.dofs.n_p) == 0
        assert L.nsx_eval_probes(h, None, None, None, None) == -1
        assert L.nsx_get_probe_cells(h, None, None, None) == -1
        assert b"nsx_set_probes" in L.nsx_last_error(h)
        assert L.nsx_set_probes(h, 2, pp, -1.0) == 0 and L.nsx_eval_probes(h, None, None, None, None) == 0
    finally:
        dev.close()
    # handles without a mesh (raw calls, as tests/test_abi.py makes them)
    L = nsx.lib()
    h = ctypes.c_void_p()
    prm = nsx.Params(2, 0, 1e-3, 1e-2)
    assert L.nsx_create(ctypes.byref(prm), ctypes.byref(h)) == 0
    try:
        assert L.nsx_set_probes(h, 2, pp, -1.0) == -1                                # neither tables nor mesh
        t = p.tables
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.N2, t.dN2, t.N1, t.weights)]
        # a (dim, n_p2) other than (2, 6) / (3, 10) never gets as far as a mesh: nsx_set_tables refuses it with NSX_ERR_UNSUPPORTED, and the
        # probe calls' own check of the pair stands behind that one
        assert L.nsx_set_tables(h, t.n_q, 10, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == -3
        assert L.nsx_set_probes(h, 2, pp, -1.0) == -1
        assert L.nsx_set_tables(h, t.n_q, t.n_p2, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == 0
        assert L.nsx_set_probes(h, 2, pp, -1.0) == -1                                # tables, no mesh
        assert b"nsx_set_mesh" in L.nsx_last_error(h)
        assert L.nsx_get_probe_cells(h, None, None, None) == -1 and L.nsx_eval_probes(h, None, None, None, None) == -1
    finally:
        L.nsx_destroy(h)


# ---------------------------------------------------------------------------------------------- 8. distributed
def test_distributed_probes_have_one_owner_and_every_rank_the_same_values(tmp_path):
    """3D cylinder level 1 on 2 processes (one card, gloo, host callbacks) with 2 sub-ranks each, the launch recipe of
    tests/test_gpu_diagnostics.py::test_distributed_diagnostics_count_every_cell_once on a master port of its own."""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    import probes_dist_worker as W
    dim, level, world, n_sub = 3, 1, 2, 2
    prefix = str(tmp_path / "probes")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29597", os.path.join(ROOT, "tests", "probes_dist_worker.py"), str(dim), str(level), str(n_sub), prefix]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [np.load("%s_rank%d.npz" % (prefix, k)) for k in range(world)]
    # the single-process handle on the same mesh, numbering and rank table
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    pts, w = W.points(mesh, dofs, world)
    assert len(pts[w["shared"]]) == 50
    state = W.state(dofs)
    ref = PR.evaluate(mesh, dofs, state, pts)
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4)
    try:
        dev.set_solution(state)
        dev.set_probes(pts)
        one = dev.eval_probes(gradient=True)
    finally:
        dev.close()
    r0 = ranks[0]
    for d in ranks[1:]:
        for k in ("owners", "found", "velocity", "pressure", "gradient"):
            assert np.array_equal(d[k], r0[k]), k                                    # every rank holds the same bits
    assert np.array_equal(r0["found"], one["found"]) and np.array_equal(r0["found"], ref["found"])
    owners = r0["owners"]
    assert np.array_equal(owners >= 0, r0["found"]) and set(owners[r0["found"]].tolist()) == set(range(world))
    n_owned = np.zeros(len(pts), dtype=int)
    for k, d in enumerate(ranks):
        mine = d["cells"] >= 0
        n_owned += mine
        assert np.array_equal(mine, owners == k)                                     # cells is -1 where another rank owns the probe
        assert (d["cells"][mine] < int(d["n_layer1"])).all()                         # the owner holds the cell in its layer-1 list
        gcell = d["cell_ids"][d["cells"][mine]]                                      # ... and it is a cell that contains the point
        X = np.asarray(mesh.vertices, dtype=np.longdouble)[np.asarray(mesh.cells)[gcell]]
        lam = d["lam"][mine].astype(np.longdouble)
        assert np.abs(np.einsum("nv,nvd->nd", lam, X) - pts[mine]).max() < 1e-13 and lam.min() >= -1e-12
        before, mid, after = d["counters"]
        assert mid[0] - before[0] == 1 and after[0] - mid[0] == 1                     # one all-reduce per call ...
        assert before[1] == mid[1] == after[1]                                       # ... and no ghost exchange
    assert np.array_equal(n_owned, r0["found"].astype(int))                          # exactly one owner per found point
    assert r0["found"][w["shared"]].all() and r0["found"][w["support"]].all() and not r0["found"][w["outside"]].any()
    got = {k: r0[k] for k in ("velocity", "pressure", "gradient")}
    check("cylinder3d-l1-w2x2", "probes_distributed", got, ref, grad_mask=ref["mult"] == 1)
    check("cylinder3d-l1-w2x2-vs-one", "probes_distributed", {k: got[k] for k in ("velocity", "pressure")}, dict(ref, velocity=one["velocity"], pressure=one["pressure"]))
    for k in ("velocity", "pressure", "gradient"):
        assert not got[k][~r0["found"]].any()


# ---------------------------------------------------------------------------------------------- 9. executable
def test_executable_writes_the_pressure_series_only_when_asked(tmp_path):
    """navier_stokes2D level:1 3 4 with NSX_PROBES=1 appends one row per step to pressure_difference_2D.csv; its last row is what
    Nsx.eval_probes() gives behind the same three steps driven from Python (the recipe of tests/test_gpu_executables.py)."""
    import __graft_entry__ as ge
    ge.build()
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    dim = 2
    exe = os.path.join(ROOT, "navierstokes_project_nm4pde_amd", "host", "navier_stokes%dD" % dim)
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    env = {k: v for k, v in os.environ.items() if k != "NSX_PROBES"}
    out = subprocess.run([exe, "level:1", "3", "4"], cwd=with_dir, env=dict(env, NSX_PROBES="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain = subprocess.run([exe, "level:1", "3", "4"], cwd=without_dir, env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    assert not (without_dir / "pressure_difference_2D.csv").exists()

    def untimed(text):
        return [line for line in text.splitlines() if not re.search(r"[Tt]ime taken|seconds|elapsed", line)]
    assert untimed(out.stdout) == untimed(plain.stdout) and len(untimed(out.stdout)) > 10
    rows = np.loadtxt(with_dir / "pressure_difference_2D.csv", delimiter=",")
    assert rows.shape == (3, 5) and rows[:, 0].astype(int).tolist() == [1, 2, 3] and np.allclose(rows[:, 1], [0.01, 0.02, 0.03])
    assert np.array_equal(rows[:, 4], rows[:, 2] - rows[:, 3])
    mesh = Mesh.cylinder(dim, 1).partition(1, 4)
    dofs, tables = DoFs(mesh, "colour"), Tables(dim)
    dt = 0.01
    dev = nsx.Nsx(dofs, tables, 1e-3, dt)
    try:
        dev.set_solution(np.zeros(dofs.n_dofs))
        dev.set_probes(PR.pressure_points(dim))
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
        ev = dev.eval_probes()
        ref = PR.evaluate(mesh, dofs, dev.solution, PR.pressure_points(dim))
    finally:
        dev.close()
    assert ev["found"].all()
    for k in range(2):
        assert abs(rows[2, 2 + k] - ev["pressure"][k]) <= TOL * ref["S_p"][k], (k, rows[2, 2 + k], ev["pressure"][k])
    assert abs(rows[2, 4] - (ev["pressure"][0] - ev["pressure"][1])) <= TOL * (ref["S_p"][0] + ref["S_p"][1])
