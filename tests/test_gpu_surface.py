"""GPU suite: the surface loads (include/nsx.h: nsx_set_surface / nsx_compute_surface / nsx_get_surface_field; csrc/nsx_surface.hip) against
closed forms, against the extended-precision restatement tests/surface_reference.py (itself pinned by tests/test_surface_reference.py) and
against nsx_compute_forces.

Tolerances: every field at the face nodes and at the surface nodes |delta| <= 1e-12 X, the project's standing 1e-12 scaled by the helper's sum
of the absolute terms in the library's order of evaluation (where X vanishes the value has to be exactly 0); every total
|delta| <= (C1 + fold depth) 2^-53 A, the bound derived in surface_reference's docstring.
Shapes: the 2D box has 12 faces and 36 face nodes (less than one wave), the 3D box more than one wave of faces ending in a partial one, the
2D cylinder at level 1 exactly one wave (64 faces in groups of 6, 6, 36 and 16), the 3D cylinder at level 1 968 faces in groups of 48, 48, 744
and 128 (the fold of the third takes two levels), patches of 1 to 7 faces and 70 cells with two boundary faces.
Measured maxima go to conftest.record (DESIGN.md quotes them).  Tests need a real MI355X."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import diagnostics_reference as R
import nodal_reference as NR
import probe_reference as PR
import surface_reference as SR
import test_surface_reference as TSR
from conftest import Problem, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
_f64p, _i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
CENTRE = {2: [0.2, 0.2], 3: [0.5, 0.2, 0.205]}                                          # the cylinder's axis


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2 if p.dim == 3 else 3), time)


def faces_of(p, ids=None):
    from navierstokes_project_nm4pde_amd.problem import boundary_faces
    return boundary_faces(p.mesh, ids)


def fields(dev):
    """every field of the last compute: {"faces": {name: [nf][npf][nc]}, "nodes": {name: [ns][nc]}}"""
    from navierstokes_project_nm4pde_amd import nsx
    return {"faces": {name: dev.surface_field(k, nsx.SURFACE_AT_FACES) for k, name in enumerate(SR.FIELDS)},
            "nodes": {name: dev.surface_field(k, nsx.SURFACE_AT_NODES) for k, name in enumerate(SR.NODE_FIELDS)}}


def totals_arrays(totals, dim):
    """the list of dicts of compute_surface() shaped as the helper's totals; the entries the dimension does not use have to be 0"""
    out = {k: np.array([t[k] for t in totals]) for k in ("area", "flux", "pressure_integral", "n_faces")}
    for k in ("force_pressure", "force_viscous"):
        v = np.array([t[k] for t in totals])
        assert not v[:, dim:].any()
        out[k] = v[:, :dim]
    tq = np.array([t["torque"] for t in totals])
    assert dim == 3 or not tq[:, :2].any()
    out["torque"] = tq if dim == 3 else tq[:, 2:]
    return out


def same_bits(a, b, what=""):
    for at in ("faces", "nodes"):
        for k in a[at]:
            assert np.array_equal(a[at][k], b[at][k], equal_nan=True), (what, at, k)


def same_totals(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def check_fields(name, test, got, ref):
    m = {}
    for at in ("faces", "nodes"):
        for k in got[at]:
            assert np.isfinite(ref[at + "_X"][k]).all(), (name, at, k)                   # every entry has a finite bound: none is exempted
            m[at + "_" + k] = SR.field_ratio(got[at][k], ref[at][k], ref[at + "_X"][k])
    print(name, {k: "%.2e" % v for k, v in m.items()})
    record(test, case=name, **m)
    for k, v in m.items():
        assert v <= TOL, (name, k, v)


def check_totals(name, test, tot, ref):
    m = {}
    for k in SR.TOTALS:
        d, b = np.abs(tot[k] - ref["totals"][k]), SR.total_bound(ref, k)
        m[k] = float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d == 0, 0.0, np.inf))))
    print(name, "totals / bound", {k: "%.2e" % v for k, v in m.items()})
    record(test, case=name, **m)
    for k, v in m.items():
        assert v <= 1.0, (name, k, v)
    assert np.array_equal(tot["n_faces"], ref["n_faces"])


def run(dev, p, state, cells, lfs, groups, form, centre, n_groups=None):
    """set, compute, read everything back, and the helper on the same input"""
    dev.set_solution(state)
    dev.set_surface(cells, lfs, groups, n_groups, form, centre)
    tot = totals_arrays(dev.compute_surface(), p.dim)
    got = fields(dev)
    ref = SR.surface(p.mesh, p.dofs, state, cells, lfs, groups, n_groups=n_groups, nu=p.nu, form=form, centre=centre)
    info, lay = dev.surface_info(), dev.surface_layout()
    assert info == {"n_faces": len(cells), "n_groups": len(ref["n_faces"]), "n_nodes": len(ref["layout"]["nodes"]), "nodes_per_face": 3 if p.dim == 2 else 6}
    assert np.array_equal(lay["nodes"], ref["layout"]["nodes"]) and np.array_equal(lay["node_groups"], ref["layout"]["node_groups"])
    assert np.array_equal(lay["face_nodes"], ref["layout"]["face_nodes"])
    assert (np.abs(lay["areas"] - ref["areas"]) <= SR.C1 * 2.0 ** -53 * ref["areas_X"]).all()
    return tot, got, ref


# ---------------------------------------------------------------------------------------------- 1. closed form
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("form", [SR.SYMMETRIC, SR.GRADIENT])
def test_quadratic_state_on_the_box_gives_the_closed_forms(dim, form):
    """all boundary faces of the box meshes of tests/test_surface_reference.py: the analytic pressure, traction and shear at every face
    node, the helper at every face node and surface node, the totals per group against the helper and summed against the divergence theorem"""
    p = Problem("box", dim, nu=0.05)
    cells, lfs, groups = faces_of(p)
    assert len(cells) == (12 if dim == 2 else len(cells)) and len(cells) % 64 != 0 and (dim == 2) == (len(cells) < 64)
    centre = [0.3, 0.7, 0.2][:dim]
    state = PR.quadratic_state(p.dofs, TSR.G_P)
    dev = p.device()
    try:
        tot, got, ref = run(dev, p, state, cells, lfs, groups, form, centre)
        nc = ctypes.c_int(0)
        for which, want in enumerate((1, dim, dim, 1, dim, 1)):
            assert dev.L.nsx_surface_field_components(dev._h, which, ctypes.byref(nc)) == 0 and nc.value == want
    finally:
        dev.close()
    tag = "box%dd-form%d" % (dim, form)
    check_fields(tag, "surface_closed_form_helper", got, ref)
    check_totals(tag, "surface_closed_form_totals", tot, ref)
    # the analytic values at the face nodes, with the helper's normal (a box: an axis, exact)
    _, G = R.quadratic_field(ref["x"].reshape(-1, dim).astype(np.longdouble))
    G = G.astype(np.float64).reshape(ref["G"].shape)
    n = ref["faces"]["normal"]
    pr = (7.0 + ref["x"] @ np.array(TSR.G_P[:dim]))[:, :, None]
    tau = p.nu * (G + np.swapaxes(G, 2, 3)) if form == SR.SYMMETRIC else p.nu * G
    tn = (tau * n[:, :, None, :]).sum(axis=3)
    exact = {"pressure": pr, "traction": pr * n - tn, "shear": -(tn - (n * tn).sum(axis=2, keepdims=True) * n), "normal": n}
    exact["shear_magnitude"] = np.linalg.norm(exact["shear"], axis=2, keepdims=True)
    m = {k: SR.field_ratio(got["faces"][k], v, ref["faces_X"][k] + 4 * 2.0 ** -53 * np.abs(v) / TOL) for k, v in exact.items()}
    print(tag, "analytic", {k: "%.2e" % v for k, v in m.items()})
    record("surface_closed_form", case=tag, **m)
    for k, v in m.items():
        assert v <= TOL, (k, v)
    TSR.check_closed_forms(dim, ref, tot, p.nu, form, centre)                        # summed over the groups: the divergence theorem


# ---------------------------------------------------------------------------------------------- 2. parity with the helper
@pytest.mark.parametrize("dim,level", [(3, 1), (2, 2)])
def test_parity_with_the_helper(dim, level):
    p = Problem("cylinder", dim, level)
    cells, lfs, groups = faces_of(p)
    u = p.smooth_velocity()
    dev = p.device()
    try:
        tot, got, ref = run(dev, p, u, cells, lfs, groups, SR.SYMMETRIC, CENTRE[dim], n_groups=4)
    finally:
        dev.close()
    if (dim, level) == (3, 1):
        assert ref["n_faces"].tolist() == [48, 48, 744, 128] and (np.bincount(cells) == 2).sum() == 70
    obstacle = ref["layout"]["node_groups"] == 3                                     # against a vacuous pass
    assert (np.abs(got["nodes"]["shear"][obstacle]).max(axis=1) > 0).mean() > 0.9
    want = 2 * np.pi * 0.05 * (0.41 if dim == 3 else 1.0)
    assert abs(tot["area"][3] - want) <= 0.01 * want
    assert all(np.isfinite(v).all() for v in got["faces"].values()) and (got["faces"]["yplus"] > 0).mean() > 0.9
    tag = "cylinder%dd-l%d" % (dim, level)
    check_fields(tag, "surface_parity", got, ref)                                    # every face node and surface node, every field
    check_totals(tag, "surface_parity_totals", tot, ref)


# ---------------------------------------------------------------------------------------------- 3. cross-check with nsx_compute_forces
@pytest.mark.parametrize("dim", [2, 3])
def test_obstacle_force_equals_compute_forces(dim):
    """2D, NSX_SURFACE_GRADIENT: pressure + viscous force = (drag, lift) of nsx_compute_forces, whose 2D formula is (nu grad u - p I) n with
    the inward normal; both integrate a polynomial integrand exactly.  3D (its viscous formula is the reference's tangential shortcut):
    zero velocity, so that the pressure force alone is compared."""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import Tables
    p = Problem("cylinder", dim, 1)
    cells, lfs, groups = faces_of(p, [3])
    assert len(cells) == (16 if dim == 2 else 128)
    u = p.smooth_velocity()
    if dim == 3:
        u[:p.dofs.n_u] = 0.0
    dev = p.device()
    try:
        tot, got, ref = run(dev, p, u, cells, lfs, groups, SR.GRADIENT, CENTRE[dim])
        dev.set_force_faces(cells, lfs, Tables(dim, Tables.FACE))
        drag, lift = dev.compute_forces()
    finally:
        dev.close()
    force = (tot["force_pressure"] + tot["force_viscous"])[0]
    A = (ref["totals_A"]["force_pressure"] + ref["totals_A"]["force_viscous"])[0]
    d = np.abs(force[:2] - np.array([drag, lift]))
    print("forces %dd: surface %r, compute_forces %r, |delta| / A = %r" % (dim, force[:2], (drag, lift), d / A[:2]))
    record("surface_vs_forces", dim=dim, dx=float(d[0] / A[0]), dy=float(d[1] / A[1]))
    assert abs(drag) > 1e-6 and abs(lift) > 1e-9 and (d <= TOL * A[:2]).all()
    if dim == 3:
        assert not tot["force_viscous"].any()
    check_totals("obstacle%dd" % dim, "surface_obstacle_totals", tot, ref)


# ---------------------------------------------------------------------------------------------- 4. purity and reproducibility
def test_the_calls_change_no_state_and_two_calls_agree_bitwise():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    cells, lfs, groups = faces_of(p)
    assert len(cells) == 64 and np.bincount(groups).tolist() == [6, 6, 36, 16]         # exactly one wave of faces
    u = p.smooth_velocity()
    dev, twin = p.device(), p.device()
    try:
        for h in (dev, twin):
            h.set_solution(u)
        dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, CENTRE[2])
        t0 = totals_arrays(dev.compute_surface(), 2)
        f0 = fields(dev)
        for h in (dev, twin):
            h.assemble(nsx.TEMAM)
            h.apply_boundary_values(*_bc(p, p.deltat))
        same_bits(fields(dev), f0, "no recompute behind the caller's back")
        t1 = totals_arrays(dev.compute_surface(), 2)                                     # between the boundary values and the solve
        f1 = fields(dev)
        same_totals(totals_arrays(dev.compute_surface(), 2), t1, "second call")
        same_bits(fields(dev), f1, "second call")
        dev.compute_surface(totals=False)
        same_bits(fields(dev), f1, "without totals")
        assert not np.array_equal(f0["faces"]["traction"], f1["faces"]["traction"])      # the Dirichlet values are in `solution` now
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.rhs, twin.rhs)
        sa = dev.solve_time_step(nsx.YOSIDA)
        sb = twin.solve_time_step(nsx.YOSIDA)
        for key in ("outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "status"):
            assert sa[key] == sb[key], key
        assert sa["final_residual"] == sb["final_residual"]
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.solution_owned, twin.solution_owned)
        assert np.array_equal(dev.rhs, twin.rhs)
        same_bits(fields(dev), f1, "behind the solve")                                   # still the values of the last compute
        dev.set_solution(u)
        same_bits(fields(dev), f1, "behind set_solution")
        same_totals(totals_arrays(dev.compute_surface(), 2), t0, "the first state again")
        same_bits(fields(dev), f0, "the first state again")
        sol = twin.solution
        dev.set_solution(sol)
        tot = totals_arrays(dev.compute_surface(), 2)
        got = fields(dev)
        ref = SR.surface(p.mesh, p.dofs, sol, cells, lfs, groups, n_groups=4, nu=p.nu, form=SR.SYMMETRIC, centre=CENTRE[2])
        check_fields("cylinder2d-l1-solved", "surface_after_solve", got, ref)
        check_totals("cylinder2d-l1-solved", "surface_after_solve_totals", tot, ref)
    finally:
        dev.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 5. layout independence
def test_layout_and_rank_tables_change_no_bit():
    """plain, 4 sub-ranks (another numbering of the same mesh: the surface nodes mapped node by node), and internal layouts in first-touch and
    in colour order, each computed on a fresh handle and again behind a switch of the layout on that handle"""
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 3, 1)
    p4 = Problem("cylinder", 3, 1, n_sub=4)
    assert np.array_equal(p.mesh.cells, p4.mesh.cells) and np.array_equal(p.mesh.vertices, p4.mesh.vertices)
    cells, lfs, groups = faces_of(p)
    assert len(cells) == 968
    u = p.smooth_velocity()
    u4 = np.zeros_like(u)
    u4[np.asarray(p4.dofs.cell_dofs).ravel()] = u[np.asarray(p.dofs.cell_dofs).ravel()]   # the same state, dof by dof
    node4 = np.zeros(p.dofs.n_u // 3, dtype=np.int64)
    node4[NR.cell_nodes(p.dofs).ravel()] = NR.cell_nodes(p4.dofs).ravel()                 # node of p -> the same node in p4's numbering

    def once(dev, state):
        dev.set_solution(state)
        tot = totals_arrays(dev.compute_surface(), 3)
        return tot, fields(dev)
    results = []
    dev = p.device()
    try:
        dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, CENTRE[3])
        lay = dev.surface_layout()
        results.append(("plain",) + once(dev, u))
    finally:
        dev.close()
    dev = p4.device()
    try:
        dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, CENTRE[3])
        lay4 = dev.surface_layout()
        where = {(int(g), int(n)): s for s, (g, n) in enumerate(zip(lay4["node_groups"], lay4["nodes"]))}
        to4 = np.array([where[(int(g), int(node4[n]))] for g, n in zip(lay["node_groups"], lay["nodes"])])
        assert len(lay4["nodes"]) == len(lay["nodes"]) and len(set(to4.tolist())) == len(to4)
        tot, got = once(dev, u4)
        got["nodes"] = {k: v[to4] for k, v in got["nodes"].items()}
        results.append(("ranks4", tot, got))
    finally:
        dev.close()
    for first, second in ((nsx.FIRST_TOUCH, nsx.COLOUR), (nsx.COLOUR, nsx.FIRST_TOUCH)):
        dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, first, 0))
        try:
            assert dev.layout_info()["on"] and dev.layout_info()["ranks"] == 8
            dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, CENTRE[3])
            results.append(("layout-%d" % first,) + once(dev, u))
            dev.set_internal_layout(8, second, 0)                                        # the state vectors are reset: hand the state over again
            same_bits(fields(dev), results[-1][2], "set and results outlive the switch")
            results.append(("layout-%d-to-%d" % (first, second),) + once(dev, u))
        finally:
            dev.close()
    assert len(results) == 6
    for name, tot, got in results[1:]:
        same_bits(got, results[0][2], name)
        same_totals(tot, results[0][1], name)


# ---------------------------------------------------------------------------------------------- 6. not finite
def test_a_nan_shows_up_in_exactly_the_faces_nodes_and_groups_that_hold_it():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 3, 1)
    cells, lfs, groups = faces_of(p)
    cn = NR.cell_nodes(p.dofs)
    for f in np.flatnonzero(groups == 3):                                               # the first obstacle vertex away from the walls
        node = int(cn[cells[f], SR.face_local_nodes(3)[lfs[f]][0]])
        hit = (cn[cells] == node).any(axis=1)                                           # the faces whose cell holds the node
        if set(groups[hit].tolist()) == {3}:
            break
    dof = 3 * node + 1                                                                  # its second velocity component
    assert 2 <= hit.sum() <= len(cells) // 4 and set(groups[hit].tolist()) == {3}
    u = p.smooth_velocity()
    bad = u.copy()
    bad[dof] = float("nan")
    dev = p.device()
    try:
        dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, CENTRE[3])
        dev.set_solution(u)
        t_clean = totals_arrays(dev.compute_surface(), 3)
        clean = fields(dev)
        lay = dev.surface_layout()
        dev.set_solution(bad)
        t = (nsx.SurfaceTotals * 4)()
        assert dev.L.nsx_compute_surface(dev._h, t) == 0                                 # the values propagate, the call succeeds
        t_bad = totals_arrays([g.as_dict() for g in t], 3)
        got = fields(dev)
    finally:
        dev.close()
    node_hit = np.zeros(len(lay["nodes"]), dtype=bool)
    node_hit[lay["face_nodes"][hit].ravel()] = True                                     # a hit face in the patch
    assert 0 < node_hit.sum() < len(node_hit) // 4
    finite_f = np.logical_and.reduce([np.isfinite(v).all(axis=2) for v in got["faces"].values()])    # [nf][npf]
    finite_n = np.logical_and.reduce([np.isfinite(v).all(axis=1) for v in got["nodes"].values()])
    assert np.array_equal(~finite_f, np.repeat(hit[:, None], 6, axis=1)) and np.array_equal(~finite_n, node_hit)
    for k in ("traction", "shear", "shear_magnitude", "yplus"):
        assert np.isnan(got["faces"][k][hit]).all(), k
    assert np.isfinite(got["faces"]["pressure"]).all() and np.isfinite(got["faces"]["normal"]).all()
    for k, v in got["faces"].items():
        assert np.array_equal(v[~hit], clean["faces"][k][~hit]), k                       # every other value: the clean run's bits
    for k, v in got["nodes"].items():
        assert np.array_equal(v[~node_hit], clean["nodes"][k][~node_hit]), k
    for k in t_bad:
        assert np.array_equal(t_bad[k][:3], t_clean[k][:3]), k                           # the groups without a hit face
    assert np.isnan(t_bad["force_viscous"][3]).all() and np.isnan(t_bad["torque"][3]).all()
    assert t_bad["area"][3] == t_clean["area"][3] and t_bad["n_faces"][3] == 128


# ---------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    cells, lfs, groups = (np.ascontiguousarray(a, dtype=np.int32) for a in faces_of(p))
    nf = len(cells)
    cen = np.array(CENTRE[2])
    buf = np.full((nf, 3, 2), 7.0)
    bp, nc, info = buf.ctypes.data_as(_f64p), ctypes.c_int(-5), (ctypes.c_int * 4)(-5, -5, -5, -5)
    tot = (nsx.SurfaceTotals * 4)()
    tot[0].area = 7.0
    c, l, g = (a.ctypes.data_as(_i32p) for a in (cells, lfs, groups))
    cp = cen.ctypes.data_as(_f64p)
    dev = p.device()
    try:
        L, h = dev.L, dev._h

        def refused(rc, *words):
            assert rc == -1, rc
            for w in words:
                assert w in L.nsx_last_error(h), (w, L.nsx_last_error(h))
        # no set yet
        refused(L.nsx_compute_surface(h, tot), b"nsx_compute_surface", b"nsx_set_surface first")
        refused(L.nsx_surface_info(h, info), b"nsx_set_surface first")
        refused(L.nsx_get_surface_layout(h, None, None, None, None), b"nsx_set_surface first")
        refused(L.nsx_get_surface_field(h, 0, 0, bp), b"nsx_get_surface_field")
        refused(L.nsx_surface_field_components(h, 0, ctypes.byref(nc)), b"nsx_surface_field_components")
        for fn in (L.nsx_surface_info, L.nsx_compute_surface):
            assert fn(None, None) == -1
        assert L.nsx_set_surface(None, nf, c, l, g, 4, 0, cp) == -1 and L.nsx_get_surface_field(None, 0, 0, bp) == -1
        # a good set, compute before get
        assert L.nsx_set_surface(h, nf, c, l, g, 4, 0, cp) == 0
        refused(L.nsx_get_surface_field(h, 0, 0, bp), b"nsx_compute_surface first")
        refused(L.nsx_surface_field_components(h, 0, ctypes.byref(nc)), b"nsx_compute_surface first")
        dev.set_solution(p.smooth_velocity())
        first = totals_arrays(dev.compute_surface(), 2)
        kept = fields(dev)
        # bad sets: each refused, the earlier set and its results stay
        def bad_set(words, n=nf, cc=cells, ll=lfs, gg=groups, ng=4, form=0, centre=cen, null=()):
            args = [None if k in null else a.ctypes.data_as(_i32p) for k, a in enumerate((cc, ll, gg))]
            refused(L.nsx_set_surface(h, n, args[0], args[1], args[2], ng, form, None if centre is None else centre.ctypes.data_as(_f64p)), b"nsx_set_surface", *words)
        def with_entry(a, k, v):
            b = a.copy()
            b[k] = v
            return b
        bad_set([b"n_faces"], n=-1)
        bad_set([b"null"], null=(0,))
        bad_set([b"null"], null=(1,))
        bad_set([b"bad cell"], cc=with_entry(cells, 5, p.dofs.n_cells))
        bad_set([b"bad cell"], cc=with_entry(cells, 5, -1))
        bad_set([b"local face"], ll=with_entry(lfs, 7, 3))
        bad_set([b"local face"], ll=with_entry(lfs, 7, -1))
        bad_set([b"group"], gg=with_entry(groups, 9, 4))
        bad_set([b"group"], gg=with_entry(groups, 9, -1))
        bad_set([b"n_groups"], ng=0)
        bad_set([b"n_groups"], ng=65)
        bad_set([b"form"], form=2)
        bad_set([b"form"], form=-1)
        bad_set([b"centre"], centre=np.array([0.2, np.nan]))
        bad_set([b"centre"], centre=np.array([np.inf, 0.2]))
        bad_set([b"twice"], cc=with_entry(cells, 1, cells[0]), ll=with_entry(lfs, 1, lfs[0]))
        # bad gets
        for which in (-1, nsx.SURFACE_FIELD_COUNT, 99):
            refused(L.nsx_get_surface_field(h, which, 0, bp), b"nsx_get_surface_field", b"field")
            refused(L.nsx_surface_field_components(h, which, ctypes.byref(nc)), b"field")
        for at in (-1, 2):
            refused(L.nsx_get_surface_field(h, 0, at, bp), b"at =")
        refused(L.nsx_get_surface_field(h, nsx.SURFACE_YPLUS, nsx.SURFACE_AT_NODES, bp), b"faces only")
        refused(L.nsx_get_surface_field(h, 0, 0, None), b"null")
        refused(L.nsx_surface_field_components(h, 0, None), b"null")
        refused(L.nsx_surface_info(h, None), b"null")
        assert (buf == 7.0).all() and nc.value == -5 and list(info) == [-5] * 4 and tot[0].area == 7.0   # a refused call writes nothing ...
        same_bits(fields(dev), kept, "earlier results stay readable")                    # ... and leaves the earlier results readable
        assert dev.surface_info()["n_faces"] == nf
        same_totals(totals_arrays(dev.compute_surface(), 2), first, "the earlier set is still installed")
        # groups = NULL: all faces in group 0; centre = NULL: the origin
        assert L.nsx_set_surface(h, nf, c, l, None, 1, 1, None) == 0
        one = dev.compute_surface()
        assert len(one) == 1 and one[0]["n_faces"] == nf and abs(one[0]["area"] - first["area"].sum()) <= 1e-14 * first["area"].sum()
        # n_faces = 0 clears the set
        assert L.nsx_set_surface(h, 0, None, None, None, 0, 9, None) == 0
        refused(L.nsx_compute_surface(h, tot), b"nsx_set_surface first")
        refused(L.nsx_get_surface_field(h, 0, 0, bp), b"nsx_set_surface first")
        # a second nsx_set_mesh drops the set
        assert L.nsx_set_surface(h, nf, c, l, g, 4, 0, cp) == 0 and L.nsx_compute_surface(h, None) == 0
        cd = np.ascontiguousarray(p.dofs.cell_dofs, dtype=np.int32)
        cc = np.ascontiguousarray(p.dofs.cell_coords, dtype=np.float64)
        assert L.nsx_set_mesh(h, p.dofs.n_cells, p.dofs.dofs_per_cell, cd.ctypes.data_as(_i32p), cc.ctypes.data_as(_f64p), p.dofs.n_u, p.dofs.n_p) == 0
        refused(L.nsx_surface_info(h, info), b"nsx_set_surface first")
        refused(L.nsx_get_surface_field(h, 0, 0, bp), b"nsx_set_surface first")
        dev.set_solution(p.smooth_velocity())
        assert L.nsx_set_surface(h, nf, c, l, g, 4, 0, cp) == 0
        same_totals(totals_arrays(dev.compute_surface(), 2), first, "the same set on the new mesh")
    finally:
        dev.close()
    # handles without a mesh (raw calls, as tests/test_abi.py makes them)
    L = nsx.lib()
    h = ctypes.c_void_p()
    prm = nsx.Params(2, 0, 1e-3, 1e-2)
    assert L.nsx_create(ctypes.byref(prm), ctypes.byref(h)) == 0
    try:
        assert L.nsx_set_surface(h, nf, c, l, g, 4, 0, cp) == -1 and b"nsx_set_surface" in L.nsx_last_error(h)   # neither tables nor mesh
        t = p.tables
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.N2, t.dN2, t.N1, t.weights)]
        # a (dim, n_p2) other than (2, 6) / (3, 10) never gets as far as a mesh: nsx_set_tables refuses it with NSX_ERR_UNSUPPORTED, and the
        # surface calls' own check of the pair (post_check_space, NSX_ERR_UNSUPPORTED as well) stands behind that one
        assert L.nsx_set_tables(h, t.n_q, 10, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == -3
        assert L.nsx_set_tables(h, t.n_q, t.n_p2, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == 0
        assert L.nsx_set_surface(h, nf, c, l, g, 4, 0, cp) == -1 and b"nsx_set_mesh" in L.nsx_last_error(h)      # tables, no mesh
        assert L.nsx_compute_surface(h, None) == -1 and L.nsx_get_surface_field(h, 0, 0, bp) == -1
        assert L.nsx_surface_info(h, info) == -1 and L.nsx_surface_field_components(h, 0, ctypes.byref(nc)) == -1
    finally:
        L.nsx_destroy(h)
    assert (buf == 7.0).all()


# ---------------------------------------------------------------------------------------------- 8. distributed
def test_distributed_surface_loads(tmp_path):
    """3D cylinder level 1 on 2 processes (one card, gloo, host callbacks) with 2 sub-ranks each, the launch recipe of
    tests/test_gpu_nodal_fields.py::test_distributed_nodal_fields_equal_the_single_process_handles_bitwise on a master port of its own."""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import boundary_faces
    import surface_dist_worker as W
    dim, level, world, n_sub = 3, 1, 2, 2
    prefix = str(tmp_path / "surface")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29627", os.path.join(ROOT, "tests", "surface_dist_worker.py"), str(dim), str(level), str(n_sub), prefix]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [np.load("%s_rank%d.npz" % (prefix, k)) for k in range(world)]
    # the single-process handle on the same mesh, numbering and rank table
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    state = W.state(dofs)
    cells, lfs, groups = boundary_faces(mesh)
    assert len(cells) == 968
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4)
    try:
        dev.set_solution(state)
        dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, W.CENTRE[dim])
        dev.compute_surface()
        one, lay = fields(dev), dev.surface_layout()
    finally:
        dev.close()
    ref = SR.surface(mesh, dofs, state, cells, lfs, groups, n_groups=4, nu=1e-3, form=SR.SYMMETRIC, centre=W.CENTRE[dim])
    check_fields("cylinder3d-l1-single", "surface_distributed_single", one, ref)
    where = {(int(g), int(n)): s for s, (g, n) in enumerate(zip(lay["node_groups"], lay["nodes"]))}
    covered = np.zeros(len(lay["nodes"]), dtype=int)
    for k, d in enumerate(ranks):
        lo, hi = (int(x) for x in d["gpu_u_ptr"][k:k + 2])
        assert np.all(np.diff(d["kept"]) > 0) and 0 < len(d["kept"]) < 968               # ascending global face order, a part of the faces
        to_one = np.array([where[(int(g), int(n))] for g, n in zip(d["node_groups"], d["nodes"])])   # global node ids
        owned = (d["nodes"] >= lo) & (d["nodes"] < hi)
        assert 0 < owned.sum() < len(owned)
        covered[to_one[owned]] += 1
        for name in SR.NODE_FIELDS:
            got = d["node_" + name]
            assert np.array_equal(got[owned], one["nodes"][name][to_one[owned]]), (k, name)   # owned surface nodes: the single handle's bits
            assert not got[~owned].any(), (k, name)                                      # nothing else is filled
            assert np.array_equal(d["again_" + name], got), (k, name)                    # the compute without totals: the same values
        for name in SR.FIELDS:
            assert np.array_equal(d["face_" + name], one["faces"][name][d["kept"]]), (k, name)   # every face passed
        before, mid, after = d["counters"]
        assert tuple(mid - before) == (1, 0) and tuple(after - mid) == (0, 0)            # one all-reduce with totals, none without; no ghost exchange
    assert (covered == 1).all()                                                          # together the ranks cover every surface node exactly once
    tots = [totals_arrays([{k: d["total_" + k][g] for k in W.TOTAL_KEYS} for g in range(4)], dim) for d in ranks]
    same_totals(tots[0], tots[1], "every rank gets the same totals")
    assert tots[0]["n_faces"].tolist() == [48, 48, 744, 128] and tots[0]["n_faces"].sum() == 968
    ref["depth"] = ref["depth"] + 1                                                      # the sum over the two ranks
    check_totals("cylinder3d-l1-w2x2", "surface_distributed_totals", tots[0], ref)


# ---------------------------------------------------------------------------------------------- 9. executable
def test_executable_writes_the_surface_loads_only_when_asked(tmp_path):
    """navier_stokes2D level:1 3 4 with NSX_SURFACE=1 appends one row per time step to surface_loads_2D.csv and writes one distribution file
    per output step beside the VTU; the last row and the last file hold what Nsx.compute_surface() and surface_field() give behind the same
    three steps driven from Python (the recipe of tests/test_gpu_executables_lattice.py).  Without the variable nothing changes."""
    import re
    import __graft_entry__ as ge
    ge.build()
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, boundary_faces, cylinder_boundary_values
    dim = 2
    exe = os.path.join(ROOT, "navierstokes_project_nm4pde_amd", "host", "navier_stokes%dD" % dim)
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    env = {k: v for k, v in os.environ.items() if k not in ("NSX_SURFACE", "NSX_LATTICE", "NSX_FIELDS")}
    out = subprocess.run([exe, "level:1", "3", "4"], cwd=with_dir, env=dict(env, NSX_SURFACE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain = subprocess.run([exe, "level:1", "3", "4"], cwd=without_dir, env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr

    def untimed(text):
        return [line for line in text.splitlines() if not re.search(r"[Tt]ime taken|seconds|elapsed", line)]
    assert untimed(out.stdout) == untimed(plain.stdout) and len(untimed(out.stdout)) > 10
    new_top = sorted(set(os.listdir(with_dir)) - set(os.listdir(without_dir)))
    new_out = sorted(set(os.listdir(with_dir / "output2D_1")) - set(os.listdir(without_dir / "output2D_1")))
    assert new_top == ["surface_loads_2D.csv"] and new_out == ["surface-navier-stokes-2D_%d.csv" % k for k in range(4)]
    assert not set(os.listdir(without_dir)) - set(os.listdir(with_dir))
    bad = subprocess.run([exe, "level:1", "1", "4"], cwd=without_dir, env=dict(env, NSX_SURFACE="2"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "NSX_SURFACE" in bad.stdout + bad.stderr
    loads = np.loadtxt(with_dir / "surface_loads_2D.csv", delimiter=",", ndmin=2)
    assert loads.shape == (3, 8) and np.allclose(loads[:, 0], [0.01, 0.02, 0.03])
    rows = [np.loadtxt(with_dir / "output2D_1" / name, delimiter=",", ndmin=2) for name in new_out]
    assert all(r.shape == rows[0].shape and r.shape[1] == 7 for r in rows) and not rows[0][:, 4:].any()   # the initial condition is zero
    # the same three steps from Python
    mesh = Mesh.cylinder(dim, 1).partition(1, 4)
    dofs, tables = DoFs(mesh, "colour"), Tables(dim)
    dt = 0.01
    cells, lfs, groups = boundary_faces(mesh, [0, 1, 2, 3])
    dev = nsx.Nsx(dofs, tables, 1e-3, dt)
    try:
        dev.set_solution(np.zeros(dofs.n_dofs))
        dev.set_surface(cells, lfs, groups, 4, nsx.SURFACE_SYMMETRIC, CENTRE[dim])
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
        tot = totals_arrays(dev.compute_surface(), dim)
        got, lay = fields(dev), dev.surface_layout()
        ref = SR.surface(mesh, dofs, dev.solution, cells, lfs, groups, n_groups=4, nu=1e-3, form=SR.SYMMETRIC, centre=CENTRE[dim])
    finally:
        dev.close()
    last = loads[-1]
    pairs = [(last[1:3], "force_pressure", 3, slice(0, 2)), (last[3:5], "force_viscous", 3, slice(0, 2)), (last[5:6], "torque", 3, slice(0, 1)),
             (last[6:7], "flux", 0, None), (last[7:8], "flux", 1, None)]
    for value, key, group, comp in pairs:
        mine = tot[key][group] if comp is None else tot[key][group][comp]
        bound = SR.total_bound(ref, key)[group] if comp is None else SR.total_bound(ref, key)[group][comp]
        assert (np.abs(value - mine) <= bound).all(), (key, value, mine)
    assert abs(last[1]) > 1e-6 and abs(last[6]) > 1e-3                                    # a flow, a flow rate through the inlet
    on = lay["node_groups"] == 3
    pts = np.asarray(dofs.support_points)[lay["nodes"][on] * dim]
    file = rows[-1]
    assert len(file) == on.sum() and np.array_equal(file[:, :2], pts)
    for cols, key in ((slice(2, 4), "normal"), (slice(4, 5), "pressure"), (slice(5, 7), "shear")):
        d = np.abs(file[:, cols] - got["nodes"][key][on])
        assert (d <= TOL * ref["nodes_X"][key][on]).all(), key
    assert np.abs(file[:, 5:7]).max() > 0
