"""GPU suite: the nodal fields (include/nsx.h: nsx_compute_nodal_fields / nsx_nodal_field_components / nsx_get_nodal_field;
csrc/nsx_nodal.hip) against closed forms and against the extended-precision restatement tests/nodal_reference.py (itself pinned by
tests/test_nodal_reference.py).

Tolerance: |delta Gbar_ij| <= 1e-12 S_G,ij with the helper's absolute-term sum S_G,ij = sum_c |c| sum_a |U_a,i| |d_j N_a| / sum_c |c| -- the
project's standing 1e-12 (tests/test_gpu_probes.py), scaled by the sum of the absolute terms so that it holds under cancellation; where S
vanishes the value has to be exactly 0.  A derived field: 1e-12 times S_G propagated to first order through its formula (the helper's
S_vorticity, S_q, S_strain, S_divergence).
The kernel's tile is 64 nodes (one wave walks the patch lists of 64 nodes sorted by patch size).  The closed-form meshes have 49 (box 2D),
245 (box 3D) and 27 (cube) nodes: less than one tile, three full tiles and a partial one, less than half a tile; the cylinders have 4806
nodes in 76 tiles (3D level 1) and 1364 nodes in 22 tiles (2D level 2).  Patch sizes from 1 (a corner's own cell) to the mesh's largest (8,
32, 6, 28 and 7 cells) meet in every one of them, so tiles of long lists, of short lists and the tiles in which the length changes all run.
Measured maxima go to conftest.record (DESIGN.md quotes them).  Tests need a real MI355X."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diagnostics_reference as R
import nodal_reference as NR
import probe_reference as PR
from conftest import Problem, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
_f64p, _i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2 if p.dim == 3 else 3), time)


def fields(dev):
    """the five fields of the last compute call, shaped as the helper's"""
    dim = dev.dim
    out = {name: dev.nodal_field(k) for k, name in enumerate(NR.NAMES)}
    n = len(out["gradient"])
    assert out["gradient"].shape == (n, dim * dim) and out["vorticity"].shape == (n, 3 if dim == 3 else 1)
    out["gradient"] = out["gradient"].reshape(n, dim, dim)
    for k in ("q", "strain", "divergence"):
        assert out[k].shape == (n, 1)
        out[k] = out[k][:, 0]
    return out


def ratios(got, ref, bounds=None, prefix="S_"):
    """largest |delta| / S of every field over the nodes (0 / 0 = 0: where S vanishes the value has to be exactly 0)"""
    bounds = ref if bounds is None else bounds
    m = {}
    for k in NR.NAMES:
        d, s = np.abs(got[k] - ref[k]), np.asarray(bounds[prefix + k])
        m[k] = float(np.max(np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d == 0, 0.0, np.inf))))
    return m


def check(name, test, got, ref, bounds=None, prefix="S_"):
    m = ratios(got, ref, bounds, prefix)
    print(name, {k: "%.2e" % v for k, v in m.items()})
    record(test, case=name, **m)
    for k, v in m.items():
        assert v <= TOL, (name, k, v)
    return m


def same_bits(a, b, what=""):
    for k in NR.NAMES:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# ---------------------------------------------------------------------------------------------- 1. closed form
@pytest.mark.parametrize("kind,dim", [("box", 2), ("box", 3), ("cube", 3)])
def test_quadratic_velocity_gives_the_analytic_fields_at_every_node(kind, dim):
    """box: 18 triangles with 49 nodes (less than one tile of 64) / 108 tetrahedra with 245 nodes (three full tiles and a partial one);
    cube level 1: 6 cells, 27 nodes (fewer cells and nodes than one wave).  Every node is compared."""
    p = Problem(kind, dim, 1) if kind == "cube" else Problem(kind, dim)
    assert p.dofs.n_cells == ({2: 18, 3: 108}[dim] if kind == "box" else 6)
    state = PR.quadratic_state(p.dofs)
    ref = NR.nodal_fields(p.mesh, p.dofs, state)
    _, G = R.quadratic_field(NR.node_points(p.dofs).astype(np.longdouble))
    exact = {k: v.astype(np.float64) for k, v in NR.derive(G).items()}
    exact["gradient"] = G.astype(np.float64)
    sizes = np.bincount(NR.cell_nodes(p.dofs).ravel(), minlength=p.dofs.n_u // dim)
    assert np.array_equal(ref["patch_size"], sizes) and sizes.min() == 1 and sizes.max() > 1
    assert {1, int(sizes.max())} <= set(sizes.tolist())
    dev = p.device()
    try:
        dev.set_solution(state)
        dev.compute_nodal_fields()
        got = fields(dev)
        assert len(got["q"]) == p.dofs.n_u // dim
        check("%s%dd" % (kind, dim), "nodal_closed_form", got, exact, bounds=ref)
        check("%s%dd-helper" % (kind, dim), "nodal_closed_form_helper", got, ref)
        nc = ctypes.c_int(0)
        for which, want in enumerate((dim * dim, 3 if dim == 3 else 1, 1, 1, 1)):
            assert dev.L.nsx_nodal_field_components(dev._h, which, ctypes.byref(nc)) == 0 and nc.value == want
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 2. parity with the helper
@pytest.mark.parametrize("dim,level", [(3, 1), (2, 2)])
def test_parity_with_the_helper(dim, level):
    p = Problem("cylinder", dim, level)
    assert p.dofs.n_cells == (2832 if dim == 3 else 632)
    u = p.smooth_velocity()
    ref = NR.nodal_fields(p.mesh, p.dofs, u)
    dev = p.device()
    try:
        dev.set_solution(u)
        dev.compute_nodal_fields()
        got = fields(dev)
        assert (np.abs(got["vorticity"]).max(axis=1) > 0).mean() > 0.9                  # against a vacuous pass
        assert np.isfinite(got["gradient"]).all() and (ref["patch_size"] >= 1).all()
        check("cylinder%dd-l%d" % (dim, level), "nodal_parity", got, ref)                # every node, every field
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 3. purity and reproducibility
def test_the_call_changes_no_state_and_two_calls_agree_bitwise():
    """The closing comparison with the helper on the SOLVED state is measured against X (the absolute terms of the library's order of
    evaluation: reference derivatives first, J^-1 last), not S.  On that state S is no bound for the rounding errors: at the mid-point of a
    wall edge parallel to an axis the wall nodes carry u = 0 and the d_x N_a of the three interior nodes vanish by cancellation between the
    rows of J^-1, so S_G,00 holds 1.1e-4 there while the terms that are added and cancel are of size 35.  Measured against S the device is
    5.9e-11 off at that node and a plain double restatement of the same sums 7.2e-11; against X both are below 1e-15."""
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    u = p.smooth_velocity()
    dev, twin = p.device(), p.device()
    try:
        for h in (dev, twin):
            h.set_solution(u)
        dev.compute_nodal_fields()
        f0 = fields(dev)                                                               # before the assembly
        for h in (dev, twin):
            h.assemble(nsx.TEMAM)
            h.apply_boundary_values(*_bc(p, p.deltat))
        assert np.array_equal(fields(dev)["gradient"], f0["gradient"])                 # no recompute behind the caller's back
        dev.compute_nodal_fields()                                                     # between the boundary values and the solve
        f1 = fields(dev)
        dev.compute_nodal_fields()
        same_bits(fields(dev), f1, "second call")
        assert not np.array_equal(f0["gradient"], f1["gradient"])                      # the Dirichlet values are in `solution` now
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.rhs, twin.rhs)
        sa = dev.solve_time_step(nsx.YOSIDA)
        sb = twin.solve_time_step(nsx.YOSIDA)
        for key in ("outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "status"):
            assert sa[key] == sb[key], key
        assert sa["final_residual"] == sb["final_residual"]
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.solution_owned, twin.solution_owned)
        assert np.array_equal(dev.rhs, twin.rhs)
        same_bits(fields(dev), f1, "behind the solve")                                 # still the values of the last compute call
        dev.set_solution(u)
        same_bits(fields(dev), f1, "behind set_solution")
        dev.compute_nodal_fields()
        same_bits(fields(dev), f0, "the first state again")
        sol = twin.solution
        dev.set_solution(sol)
        dev.compute_nodal_fields()
        check("cylinder2d-l1-solved", "nodal_after_solve", fields(dev), NR.nodal_fields(p.mesh, p.dofs, sol), prefix="X_")
    finally:
        dev.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 4. layout independence
def test_layout_and_rank_tables_change_no_bit():
    """plain, 4 sub-ranks (another numbering of the same mesh: compared node by node through the cells), and internal layouts in first-touch
    and in colour order, each computed on a fresh handle and again behind a switch of the layout on that handle"""
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 3, 1)
    p4 = Problem("cylinder", 3, 1, n_sub=4)
    assert p.dofs.n_cells == 2832
    assert np.array_equal(p.mesh.cells, p4.mesh.cells) and np.array_equal(p.mesh.vertices, p4.mesh.vertices)
    u = p.smooth_velocity()
    u4 = np.zeros_like(u)
    u4[np.asarray(p4.dofs.cell_dofs).ravel()] = u[np.asarray(p.dofs.cell_dofs).ravel()]   # the same state, dof by dof
    node4 = np.zeros(p.dofs.n_u // 3, dtype=np.int64)
    node4[NR.cell_nodes(p.dofs).ravel()] = NR.cell_nodes(p4.dofs).ravel()                 # node of p -> the same node in p4's numbering
    ref = NR.nodal_fields(p.mesh, p.dofs, u)
    results = []
    dev = p.device()
    try:
        dev.set_solution(u)
        dev.compute_nodal_fields()
        results.append(("plain", fields(dev)))
    finally:
        dev.close()
    dev = p4.device()
    try:
        dev.set_solution(u4)
        dev.compute_nodal_fields()
        results.append(("ranks4", {k: v[node4] for k, v in fields(dev).items()}))
    finally:
        dev.close()
    for first, second in ((nsx.FIRST_TOUCH, nsx.COLOUR), (nsx.COLOUR, nsx.FIRST_TOUCH)):
        dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, first, 0))
        try:
            assert dev.layout_info()["on"] and dev.layout_info()["ranks"] == 8
            dev.set_solution(u)
            dev.compute_nodal_fields()
            results.append(("layout-%d" % first, fields(dev)))
            dev.set_internal_layout(8, second, 0)                                        # the state vectors are reset: hand the state over again
            same_bits(fields(dev), results[-1][1], "results outlive the switch")
            dev.set_solution(u)
            dev.compute_nodal_fields()
            results.append(("layout-%d-to-%d" % (first, second), fields(dev)))
        finally:
            dev.close()
    check("cylinder3d-l1-plain", "nodal_layout", results[0][1], ref)
    assert len(results) == 6
    for name, got in results[1:]:
        same_bits(got, results[0][1], name)


# ---------------------------------------------------------------------------------------------- 5. not finite
def test_a_nan_shows_up_in_exactly_the_nodes_whose_patch_holds_it():
    p = Problem("cylinder", 3, 1)
    cd = np.asarray(p.dofs.cell_dofs)
    u = p.smooth_velocity()
    dof = int(cd[p.dofs.n_cells // 2, 1])                                               # second velocity component of a vertex
    assert dof < p.dofs.n_u and dof % 3 == 1
    holds = NR.patch_holds(p.dofs, dof)
    assert 10 < holds.sum() < len(holds) // 4
    bad = u.copy()
    bad[dof] = float("nan")
    dev = p.device()
    try:
        dev.set_solution(u)
        dev.compute_nodal_fields()
        clean = fields(dev)
        dev.set_solution(bad)
        assert dev.L.nsx_compute_nodal_fields(dev._h) == 0                               # the values propagate, the call succeeds
        got = fields(dev)
        assert np.array_equal(~np.isfinite(got["gradient"]).all(axis=(1, 2)), holds)
        assert np.isnan(got["gradient"][holds, 1, :]).all() and np.isfinite(got["gradient"][:, [0, 2], :]).all()
        for k in NR.NAMES:
            assert np.array_equal(got[k][~holds], clean[k][~holds]), k                   # every other node: the clean run's bits
        for k in ("q", "strain", "divergence"):
            assert np.isnan(got[k][holds]).all(), k
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 6. argument errors
def test_argument_errors():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    n_nodes = p.dofs.n_u // 2
    buf, nc = np.full((n_nodes, 4), 7.0), ctypes.c_int(-5)
    bp = buf.ctypes.data_as(_f64p)
    dev = p.device()
    try:
        L, h = dev.L, dev._h
        assert L.nsx_get_nodal_field(h, nsx.FIELD_Q, bp) == -1                           # no compute on this mesh yet
        assert b"nsx_get_nodal_field" in L.nsx_last_error(h) and b"nsx_compute_nodal_fields first" in L.nsx_last_error(h)
        assert L.nsx_nodal_field_components(h, nsx.FIELD_Q, ctypes.byref(nc)) == -1 and nc.value == -5
        assert b"nsx_nodal_field_components" in L.nsx_last_error(h)
        assert (buf == 7.0).all()
        assert L.nsx_compute_nodal_fields(None) == -1 and L.nsx_get_nodal_field(None, 0, bp) == -1
        assert L.nsx_nodal_field_components(None, 0, ctypes.byref(nc)) == -1
        dev.set_solution(p.smooth_velocity())
        assert L.nsx_compute_nodal_fields(h) == 0
        q = dev.nodal_field(nsx.FIELD_Q)
        for which in (-1, nsx.FIELD_COUNT, 99):
            assert L.nsx_get_nodal_field(h, which, bp) == -1 and b"nsx_get_nodal_field" in L.nsx_last_error(h)
            assert L.nsx_nodal_field_components(h, which, ctypes.byref(nc)) == -1
        assert L.nsx_get_nodal_field(h, nsx.FIELD_Q, None) == -1 and b"null" in L.nsx_last_error(h)
        assert L.nsx_nodal_field_components(h, nsx.FIELD_Q, None) == -1 and b"null" in L.nsx_last_error(h)
        assert (buf == 7.0).all() and nc.value == -5                                     # a refused call writes nothing ...
        assert np.array_equal(dev.nodal_field(nsx.FIELD_Q), q)                           # ... and leaves the earlier results readable
        # a second nsx_set_mesh drops the table and the results
        cd = np.ascontiguousarray(p.dofs.cell_dofs, dtype=np.int32)
        cc = np.ascontiguousarray(p.dofs.cell_coords, dtype=np.float64)
        assert L.nsx_set_mesh(h, p.dofs.n_cells, p.dofs.dofs_per_cell, cd.ctypes.data_as(_i32p), cc.ctypes.data_as(_f64p), p.dofs.n_u, p.dofs.n_p) == 0
        assert L.nsx_get_nodal_field(h, nsx.FIELD_Q, bp) == -1 and L.nsx_nodal_field_components(h, nsx.FIELD_Q, ctypes.byref(nc)) == -1
        assert b"nsx_compute_nodal_fields" in L.nsx_last_error(h)
        dev.set_solution(p.smooth_velocity())
        assert L.nsx_compute_nodal_fields(h) == 0
        assert np.array_equal(dev.nodal_field(nsx.FIELD_Q), q)
    finally:
        dev.close()
    # handles without a mesh (raw calls, as tests/test_abi.py makes them)
    L = nsx.lib()
    h = ctypes.c_void_p()
    prm = nsx.Params(2, 0, 1e-3, 1e-2)
    assert L.nsx_create(ctypes.byref(prm), ctypes.byref(h)) == 0
    try:
        assert L.nsx_compute_nodal_fields(h) == -1                                       # neither tables nor mesh
        assert b"nsx_compute_nodal_fields" in L.nsx_last_error(h)
        t = p.tables
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.N2, t.dN2, t.N1, t.weights)]
        # a (dim, n_p2) other than (2, 6) / (3, 10) never gets as far as a mesh: nsx_set_tables refuses it with NSX_ERR_UNSUPPORTED, and the
        # nodal calls' own check of the pair (NSX_ERR_UNSUPPORTED as well) stands behind that one
        assert L.nsx_set_tables(h, t.n_q, 10, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == -3
        assert L.nsx_compute_nodal_fields(h) == -1
        assert L.nsx_set_tables(h, t.n_q, t.n_p2, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == 0
        assert L.nsx_compute_nodal_fields(h) == -1                                       # tables, no mesh
        assert b"nsx_set_mesh" in L.nsx_last_error(h)
        assert L.nsx_get_nodal_field(h, 0, bp) == -1 and L.nsx_nodal_field_components(h, 0, ctypes.byref(nc)) == -1
    finally:
        L.nsx_destroy(h)


# ---------------------------------------------------------------------------------------------- 7. distributed
def test_distributed_nodal_fields_equal_the_single_process_handles_bitwise(tmp_path):
    """3D cylinder level 1 on 2 processes (one card, gloo, host callbacks) with 2 sub-ranks each, the launch recipe of
    tests/test_gpu_probes.py::test_distributed_probes_have_one_owner_and_every_rank_the_same_values on a master port of its own."""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    import nodal_dist_worker as W
    dim, level, world, n_sub = 3, 1, 2, 2
    prefix = str(tmp_path / "nodal")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29609", os.path.join(ROOT, "tests", "nodal_dist_worker.py"), str(dim), str(level), str(n_sub), prefix]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [np.load("%s_rank%d.npz" % (prefix, k)) for k in range(world)]
    # the single-process handle on the same mesh, numbering and rank table
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    state = W.state(dofs)
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4)
    try:
        dev.set_solution(state)
        dev.compute_nodal_fields()
        one = fields(dev)
    finally:
        dev.close()
    n_nodes = dofs.n_u // dim
    covered = np.zeros(n_nodes, dtype=int)
    for k, d in enumerate(ranks):
        lo, hi = (int(x) for x in d["gpu_u_ptr"][k:k + 2])
        assert 0 <= lo < hi <= n_nodes
        covered[lo:hi] += 1
        # the view keeps the layer-1 cells (the ones that hold owned nodes) in ascending global order: the fold order of the single handle
        assert np.all(np.diff(d["cell_ids"][:int(d["n_layer1"])]) > 0)
        for name in NR.NAMES:
            got = d[name].reshape((n_nodes,) + one[name].shape[1:])
            assert np.array_equal(got[lo:hi], one[name][lo:hi]), (k, name)              # owned entries: the single handle's bits
            rest = np.ones(n_nodes, dtype=bool)
            rest[lo:hi] = False
            assert not got[rest].any(), (k, name)                                        # nothing else is touched
        before, mid, after = d["counters"]
        assert tuple(before) == tuple(mid) == tuple(after)                               # no collective, no ghost exchange
    assert (covered == 1).all()                                                          # together the ranks cover every node exactly once
    check("cylinder3d-l1-w2x2", "nodal_distributed", one, NR.nodal_fields(mesh, dofs, state))


# ---------------------------------------------------------------------------------------------- 8. executable
def test_executable_writes_the_fields_only_when_asked(tmp_path):
    """navier_stokes2D level:1 3 4 with NSX_FIELDS=1 writes the arrays "vorticity" and "q_criterion" into every .vtu; without the variable
    the files hold no such array, and they are, byte for byte, the files of the run with the variable minus the two arrays."""
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(ROOT, "navierstokes_project_nm4pde_amd", "host", "navier_stokes2D")
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    env = {k: v for k, v in os.environ.items() if k != "NSX_FIELDS"}
    out = subprocess.run([exe, "level:1", "3", "4", "1"], cwd=with_dir, env=dict(env, NSX_FIELDS="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain = subprocess.run([exe, "level:1", "3", "4", "1"], cwd=without_dir, env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr

    def untimed(text):
        return [line for line in text.splitlines() if not re.search(r"[Tt]ime taken|seconds|elapsed", line)]
    assert untimed(out.stdout) == untimed(plain.stdout) and len(untimed(out.stdout)) > 10
    names = sorted(os.listdir(without_dir / "output2D_1"))
    assert names == sorted(os.listdir(with_dir / "output2D_1"))
    assert sorted(n for n in names if n.endswith(".vtu")) == ["output-navier-stokes-2D_%d.0.vtu" % k for k in range(4)]
    array = r'<P?DataArray type="Float64" Name="%s"[^>]*?(?:/>\n|>\n(.*?)</DataArray>\n)'
    moved = 0
    for name in names:
        text = (with_dir / "output2D_1" / name).read_text()
        base = (without_dir / "output2D_1" / name).read_text()
        assert "vorticity" not in base and "q_criterion" not in base
        stripped = text
        for field in ("vorticity", "q_criterion"):
            found = re.findall(array % field, text, flags=re.S)
            assert len(found) == 1, (name, field)
            stripped = re.sub(array % field, "", stripped, flags=re.S)
            if name.endswith(".vtu"):
                values = np.array(found[0].split(), dtype=float)
                assert len(values) == int(re.search(r'NumberOfPoints="(\d+)"', text).group(1)) and np.isfinite(values).all()
                if name.endswith("_0.0.vtu"):
                    assert not values.any()                                              # the initial condition is zero
                else:
                    moved += int(np.abs(values).max() > 0)
        assert stripped == base, name
    assert moved == 6                                                                    # both arrays carry a flow in all three steps
