"""GPU suite: the flow diagnostics (include/nsx.h: nsx_compute_diagnostics / nsx_get_cell_diagnostic; csrc/nsx_diag.hip) against closed
forms and against the extended-precision restatement tests/diagnostics_reference.py (itself pinned by tests/test_diagnostics_reference.py).

Tolerances:
 (a) sums (kinetic_energy, grad_l2_sq, enstrophy, change_l2^2, volume) and their per-cell shares: relative 1e-12 against the long-double
     helper -- the bound tests/test_gpu_parity.py holds forces and assembled entries to, and measured the same way (conftest.rel_err: the
     largest deviation against the largest value).  The terms are non-negative: no summation order loses more than about (terms) * eps.
 (b) div_l2 and NSX_DIAG_DIV2 are sums of squares of a quantity that itself cancels: |delta div_l2| <= 1e-12 sqrt(grad_l2_sq), and per cell
     |delta| <= 1e-12 (the cell's NSX_DIAG_GRAD2 share).
 (c) maxima: relative 1e-12.
Measured maxima go to conftest.record (DESIGN.md section 5 quotes them).  Tests need a real MI355X."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import diagnostics_reference as R
from conftest import Problem, record, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
SUM_KEYS = ("kinetic_energy", "grad_l2_sq", "enstrophy", "volume")


def _cells(dev):
    from navierstokes_project_nm4pde_amd import nsx
    return np.array([dev.cell_diagnostic(w) for w in range(nsx.DIAG_COUNT)])


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2 if p.dim == 3 else 3), time)


def _check_parity(name, d, cells, ref):
    """totals and the eight per-cell arrays of a device against the helper's; returns the measured maxima (also recorded)"""
    t, rc = ref["totals"], ref["cells"]
    grad = math.sqrt(t["grad_l2_sq"])
    m = {k: abs(d[k] - t[k]) / t[k] for k in SUM_KEYS}
    m["change2"] = abs(d["change_l2"] ** 2 - t["change_l2"] ** 2) / t["change_l2"] ** 2 if t["change_l2"] > 0 else abs(d["change_l2"])
    m["div_l2_abs_over_grad"] = abs(d["div_l2"] - t["div_l2"]) / grad
    m["cfl_max"] = abs(d["cfl_max"] - t["cfl_max"]) / t["cfl_max"]
    m["speed_max"] = abs(d["speed_max"] - t["speed_max"]) / t["speed_max"]
    for w, key in enumerate(R.KEYS):
        if w == R.DIV2:
            m["cells_div2_over_grad2"] = float(np.max(np.abs(cells[w] - rc[w]) / rc[R.GRAD2]))
        else:
            m["cells_" + key] = rel_err(cells[w], rc[w])
    print(name, {k: "%.2e" % v for k, v in m.items()})
    record("diagnostics_parity", case=name, **m)
    assert d["n_cells"] == t["n_cells"]
    for k, v in m.items():
        assert v <= TOL, (name, k, v)
    return m


# ---------------------------------------------------------------------------------------------- 1. known answer
@pytest.mark.parametrize("kind,dim", [("box", 2), ("box", 3), ("cube", 3)])
def test_quadratic_field_gives_the_closed_forms(kind, dim):
    """box: 3 x 3 (x 2) cells per side, 18 triangles / 108 tetrahedra (one full 64-lane workgroup and a partial one); cube level 1:
    fewer cells than one workgroup.  Sums against the closed forms, maxima and volume against the helper."""
    p = Problem(kind, dim, 1) if kind == "cube" else Problem(kind, dim)
    V = np.asarray(p.mesh.vertices)
    lo, hi = V.min(axis=0).tolist(), V.max(axis=0).tolist()
    ex = R.quadratic_closed_forms(hi, lo)
    u = R.interpolate_quadratic(p.dofs)
    ref = R.flow_diagnostics(p.mesh, p.dofs, p.tables, u, np.zeros_like(u), p.deltat)
    dev = p.device()
    try:
        dev.set_solution(u)
        d = dev.diagnostics()
        got = {"kinetic_energy": d["kinetic_energy"], "div2": d["div_l2"] ** 2, "grad_l2_sq": d["grad_l2_sq"], "enstrophy": d["enstrophy"]}
        m = {k: abs(got[k] - ex[k]) / ex[k] for k in got}
        m["change2"] = abs(d["change_l2"] ** 2 - 2 * ex["kinetic_energy"]) / (2 * ex["kinetic_energy"])   # previous_solution = 0
        t = ref["totals"]
        for k in ("volume", "cfl_max", "speed_max"):
            m[k] = abs(d[k] - t[k]) / t[k]
        m["volume_exact"] = abs(d["volume"] - ex["volume"]) / ex["volume"]
        print({k: "%.2e" % v for k, v in m.items()})
        record("diagnostics_known_answer", case="%s%dd" % (kind, dim), n_cells=int(d["n_cells"]), **m)
        assert d["n_cells"] == p.dofs.n_cells
        if kind == "box":
            assert p.dofs.n_cells == (108 if dim == 3 else 18)
        else:
            assert p.dofs.n_cells < 64
        for k, v in m.items():
            assert v <= TOL, (k, v)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 2. parity with the helper
@pytest.mark.parametrize("dim,level", [(3, 1), (2, 2)])
def test_parity_with_the_helper_before_and_after_a_solve(dim, level):
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", dim, level)
    u = p.smooth_velocity()
    dev = p.device()
    try:
        dev.set_solution(u)
        d0 = dev.diagnostics()
        _check_parity("cylinder%dd-l%d-set" % (dim, level), d0, _cells(dev), R.flow_diagnostics(p.mesh, p.dofs, p.tables, u, np.zeros_like(u), p.deltat))
        # one step: previous_solution = the smooth field, solution = a discretely divergence-free one
        dev.assemble(nsx.TEMAM)
        dev.apply_boundary_values(*_bc(p, p.deltat))
        prev = dev.solution                      # what solve_time_step copies into previous_solution (the Dirichlet values are in)
        st = dev.solve_time_step(nsx.YOSIDA, tol_abs=1e-10, inner_rtol=1e-8)
        assert st["status"] == 0
        d1 = dev.diagnostics()
        ref = R.flow_diagnostics(p.mesh, p.dofs, p.tables, dev.solution, prev, p.deltat)
        assert ref["totals"]["change_l2"] > 0
        _check_parity("cylinder%dd-l%d-solved" % (dim, level), d1, _cells(dev), ref)
        # the cancellation case of tolerance (b): the solve has projected the divergence the smooth field carried out of the state
        r0, r1 = d0["div_l2"] / math.sqrt(d0["grad_l2_sq"]), d1["div_l2"] / math.sqrt(d1["grad_l2_sq"])
        record("diagnostics_div_over_grad", case="cylinder%dd-l%d" % (dim, level), before=r0, after=r1)
        # NOT "far below 1": a P2/P1 solution is divergence-free against the P1 test functions only; its pointwise divergence is O(h) of
        # the second derivatives, and on these coarse meshes the ratio after the solve is of the order 0.1 (DESIGN.md section 5 quotes
        # it).  No factor between r1 and r0 follows from the discretisation, so none is asserted: the ratio falls, and the ERROR of
        # div_l2 is held to the absolute bound (b) above, which is what the cancellation is about.
        assert r1 < r0
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 3. layout invariance
def test_layout_and_rank_tables_change_no_bit():
    """The renumbering is behind the boundary, the cell-local node order is unchanged and the fold is in the caller's cell order: an
    internal layout and a table of 4 ranks give every per-cell array and every total BITWISE as the plain handle does."""
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 3, 1)
    u = R.smooth_field(p.dofs)
    results = []
    p4 = Problem("cylinder", 3, 1, n_sub=4)      # the same mesh, its nodes numbered subdomain by subdomain
    assert np.array_equal(p.mesh.cells, p4.mesh.cells) and np.array_equal(p.mesh.vertices, p4.mesh.vertices)
    u4 = np.zeros_like(u)
    u4[np.asarray(p4.dofs.cell_dofs).ravel()] = u[np.asarray(p.dofs.cell_dofs).ravel()]   # the same state, dof by dof
    for name, make, state in (("plain", lambda: p.device(), u),
                              ("layout", lambda: nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, nsx.COLOUR, 0)), u),
                              ("ranks4", lambda: p4.device(), u4)):
        dev = make()
        try:
            dev.set_solution(state)
            d = dev.diagnostics()
            results.append((name, d, _cells(dev)))
            if name == "layout":
                assert dev.layout_info()["on"] and dev.layout_info()["ranks"] == 8
            if name == "ranks4":
                assert p4.dofs.n_subdomains == 4
        finally:
            dev.close()
    _, d_ref, c_ref = results[0]
    assert d_ref["n_cells"] == p.dofs.n_cells and d_ref["kinetic_energy"] > 0
    for name, d, c in results[1:]:
        assert d == d_ref, name
        assert np.array_equal(c, c_ref), name


# ---------------------------------------------------------------------------------------------- 4. reproducibility and purity
def test_two_calls_agree_bitwise_and_the_call_changes_no_state():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 3, 1)
    u = p.smooth_velocity()
    dev, twin = p.device(), p.device()
    try:
        for h in (dev, twin):
            h.set_solution(u)
            h.assemble(nsx.TEMAM)
            h.apply_boundary_values(*_bc(p, p.deltat))
        d1, c1 = dev.diagnostics(), _cells(dev)
        d2, c2 = dev.diagnostics(), _cells(dev)
        assert d1 == d2 and np.array_equal(c1, c2)
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.solution_owned, twin.solution_owned)
        assert np.array_equal(dev.rhs, twin.rhs)
        sa = dev.solve_time_step(nsx.YOSIDA)      # the reference's tolerances: what is compared is bits, not accuracy
        sb = twin.solve_time_step(nsx.YOSIDA)
        for key in ("outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "status"):
            assert sa[key] == sb[key], key
        assert sa["final_residual"] == sb["final_residual"]
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.solution_owned, twin.solution_owned)
        # ... and between the solve and the next assembly as well
        d3 = dev.diagnostics()
        assert d3["change_l2"] > 0 and d3 != d1
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.rhs, twin.rhs)
    finally:
        dev.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 5. blow-up detection
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_value_that_is_not_finite_is_reported_and_located(bad):
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 3, 1)
    u = p.smooth_velocity()
    dof = int(np.asarray(p.dofs.cell_dofs)[p.dofs.n_cells // 2, 1])     # second velocity component of a vertex in the middle of the cell list
    assert dof < p.dofs.n_u
    u[dof] = bad
    dev = p.device()
    try:
        dev.set_solution(u)
        with pytest.raises(nsx.NsxError) as e:
            dev.diagnostics()
        assert e.value.code == -5
        assert e.value.diag is not None and not math.isfinite(e.value.diag["speed_max"])
        assert not math.isfinite(e.value.diag["kinetic_energy"])
        assert e.value.diag["n_cells"] == p.dofs.n_cells and math.isfinite(e.value.diag["volume"])
        speed = dev.cell_diagnostic(nsx.DIAG_SPEED)
        holds = (np.asarray(p.dofs.cell_dofs) == dof).any(axis=1)
        assert 0 < holds.sum() < p.dofs.n_cells
        assert np.array_equal(~np.isfinite(speed), holds)
        # the handle is not damaged: a finite state is fine again
        dev.set_solution(p.smooth_velocity())
        assert math.isfinite(dev.diagnostics()["speed_max"])
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 6. argument errors
def test_argument_errors():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    dev = p.device()
    try:
        buf = np.zeros(p.dofs.n_cells)
        ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert dev.L.nsx_get_cell_diagnostic(dev._h, nsx.DIAG_ENERGY, ptr) == -1           # nothing computed yet
        dev.set_solution(p.smooth_velocity())
        dev.diagnostics()
        assert dev.L.nsx_get_cell_diagnostic(dev._h, nsx.DIAG_ENERGY, ptr) == 0
        assert dev.L.nsx_get_cell_diagnostic(dev._h, nsx.DIAG_COUNT, ptr) == -1
        assert dev.L.nsx_get_cell_diagnostic(dev._h, -1, ptr) == -1
        assert dev.L.nsx_get_cell_diagnostic(dev._h, nsx.DIAG_ENERGY, None) == -1
        assert dev.L.nsx_compute_diagnostics(dev._h, None) == -1
        assert dev.L.nsx_compute_diagnostics(None, None) == -1
    finally:
        dev.close()
    # a handle that has its tables but no mesh (raw calls, as tests/test_abi.py makes them)
    L = nsx.lib()
    h = ctypes.c_void_p()
    prm = nsx.Params(2, 0, 1e-3, 1e-2)
    assert L.nsx_create(ctypes.byref(prm), ctypes.byref(h)) == 0
    try:
        d = nsx.FlowDiag()
        assert L.nsx_compute_diagnostics(h, ctypes.byref(d)) == -1                           # neither tables nor mesh
        t = p.tables
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.N2, t.dN2, t.N1, t.weights)]
        f64p = ctypes.POINTER(ctypes.c_double)
        assert L.nsx_set_tables(h, t.n_q, t.n_p2, t.n_p1, *[a.ctypes.data_as(f64p) for a in arrs]) == 0
        assert L.nsx_compute_diagnostics(h, ctypes.byref(d)) == -1
        assert b"nsx_set_mesh" in L.nsx_last_error(h)
    finally:
        L.nsx_destroy(h)


# ---------------------------------------------------------------------------------------------- 7. distributed
def test_distributed_diagnostics_count_every_cell_once(tmp_path):
    """3D cylinder level 1 on 2 processes (one card, gloo, host callbacks) with 2 sub-ranks each: every rank reports the totals of the
    single-process handle, every cell is counted by exactly one rank, and the call costs two all-reduces and no ghost exchange."""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    dim, level, world, n_sub = 3, 1, 2, 2
    prefix = str(tmp_path / "diag")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29591", os.path.join(ROOT, "tests", "diagnostics_dist_worker.py"), str(dim), str(level), str(n_sub), prefix]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [np.load("%s_rank%d.npz" % (prefix, k)) for k in range(world)]
    # the single-process handle on the same mesh, numbering and rank table
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4)
    try:
        dev.set_solution(R.smooth_field(dofs))
        one = dev.diagnostics()
        one_cells = _cells(dev)
    finally:
        dev.close()
    keys = list(ranks[0]["keys"])
    tot = [dict(zip(keys, d["totals"])) for d in ranks]
    for k in range(1, world):
        assert np.array_equal(ranks[k]["totals"], ranks[0]["totals"])           # every rank reports the same totals
    t = tot[0]
    assert int(t["n_cells"]) == dofs.n_cells == one["n_cells"]
    assert abs(t["volume"] - one["volume"]) <= 1e-13 * one["volume"]            # every cell exactly once
    m = {k: abs(t[k] - one[k]) / one[k] for k in SUM_KEYS}
    m["change2"] = abs(t["change_l2"] ** 2 - one["change_l2"] ** 2) / one["change_l2"] ** 2
    m["div_l2_abs_over_grad"] = abs(t["div_l2"] - one["div_l2"]) / math.sqrt(one["grad_l2_sq"])
    record("diagnostics_distributed", case="cylinder3d-l1-w2x2", **m)
    for k, v in m.items():
        assert v <= TOL, (k, v)
    assert t["cfl_max"] == one["cfl_max"] and t["speed_max"] == one["speed_max"]   # maxima: exactly
    # the ranks' counted cells partition the cell set, and a counted cell carries the single-process handle's values
    owner = np.full(dofs.n_cells, -1)
    for k, d in enumerate(ranks):
        ids, cells = d["cell_ids"], d["cells"]
        counted = cells[nsx.DIAG_VOLUME] != 0
        assert not counted[int(d["n_layer1"]):].any()                           # the counting rank holds the cell in its layer-1 list
        assert (owner[ids[counted]] == -1).all()
        owner[ids[counted]] = k
        assert (cells[:, ~counted] == 0).all()
        for w in range(nsx.DIAG_COUNT):
            assert rel_err(cells[w, counted], one_cells[w, ids[counted]]) <= TOL, (k, w)
        before, after = d["counters"]
        assert after[0] - before[0] == 2 and after[1] == before[1]
    assert (owner >= 0).all() and len(set(owner.tolist())) == world


# ---------------------------------------------------------------------------------------------- 8. executable
def test_executable_writes_the_monitor_only_when_asked(tmp_path):
    """navier_stokes2D level:1 3 4 with NSX_DIAGNOSTICS=1 appends one row per step to diagnostics_2D.csv; its last row is what
    Nsx.diagnostics() gives behind the same three steps driven from Python (the recipe of tests/test_gpu_executables.py)."""
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
    env = {k: v for k, v in os.environ.items() if k != "NSX_DIAGNOSTICS"}
    out = subprocess.run([exe, "level:1", "3", "4"], cwd=with_dir, env=dict(env, NSX_DIAGNOSTICS="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain = subprocess.run([exe, "level:1", "3", "4"], cwd=without_dir, env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    assert not (without_dir / "diagnostics_2D.csv").exists()
    rows = np.loadtxt(with_dir / "diagnostics_2D.csv", delimiter=",")
    assert rows.shape == (3, 9) and rows[:, 0].astype(int).tolist() == [1, 2, 3] and np.allclose(rows[:, 1], [0.01, 0.02, 0.03])
    mesh = Mesh.cylinder(dim, 1).partition(1, 4)
    dofs, tables = DoFs(mesh, "colour"), Tables(dim)
    dt = 0.01
    dev = nsx.Nsx(dofs, tables, 1e-3, dt)
    try:
        dev.set_solution(np.zeros(dofs.n_dofs))
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
        d = dev.diagnostics()
    finally:
        dev.close()
    for col, key in enumerate(("kinetic_energy", "div_l2", "grad_l2_sq", "enstrophy", "change_l2", "cfl_max", "speed_max"), start=2):
        assert abs(rows[2, col] - d[key]) <= 1e-9 * abs(d[key]), (key, rows[2, col], d[key])
