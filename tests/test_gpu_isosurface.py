"""GPU suite: the isosurface extraction (include/nsx.h: nsx_extract_isosurface / nsx_get_isosurface; csrc/nsx_iso.hip) against the NumPy
restatement tests/iso_reference.py (itself pinned by closed forms in tests/test_iso_reference.py), primitive by primitive in order.

Tolerance: counts and cells equal exactly; every vertex componentwise |delta x| <= 6 * 2^-53 * (|x_a| + |x_b|) -- three roundings in
t = (s_a - iso) / (s_a - s_b), one in x_b - x_a, one in the product, one in the sum, and |t (x_b - x_a)| <= |x_a| + |x_b|; the colour has the
same bound with the colour values.  The restatement computes its nodal scalars in double with the header's formulas (the device's have to be
the same doubles) and the vertices in long double from them.  Precondition of every parity case, asserted on the restatement: no nodal s lies
within 1e-9 max|s| of the isovalue, so that a rounding of sqrt cannot flip a classification.
Shapes: 18 / 108 / 6 / 2832 / 632 cells -- less than a wave, less than a workgroup, several workgroups; 4374 cells at 64 lanes give 69
workgroup totals, two passes of the scan's loop.  Measured maxima go to conftest.record (DESIGN.md quotes them).  Tests need a real MI355X."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import iso_reference as IR
import nodal_reference as NR
from conftest import Problem, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS6 = 6.0 * 2.0 ** -53
_f64p, _i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)

MESHES = {"box2d": ("box", 2, 0, 18), "box3d": ("box", 3, 0, 108), "cube1": ("cube", 3, 1, 6), "cyl3d": ("cylinder", 3, 1, 2832), "cyl2d": ("cylinder", 2, 2, 632)}
# (field, colour): every source kind as field, a different kind as colour; (kind, which, component, normal)
SOURCES = {
    "u0-pressure": ((IR.VELOCITY, 0, 0, None), (IR.PRESSURE, 0, 0, None)),
    "speed-plane": ((IR.VELOCITY, 0, -1, None), (IR.PLANE, 0, 0, [0.3, -1.0, 0.5])),
    "pressure-u1": ((IR.PRESSURE, 0, 0, None), (IR.VELOCITY, 0, 1, None)),
    "q-speed": ((IR.NODAL, 2, 0, None), (IR.VELOCITY, 0, -1, None)),
    "plane-strain": ((IR.PLANE, 0, 0, [1.0, -0.7, 0.4]), (IR.NODAL, 3, 0, None)),
}


def problem(mesh):
    kind, dim, level, n_cells = MESHES[mesh]
    p = Problem(kind, dim) if kind == "box" else Problem(kind, dim, level)
    assert p.dofs.n_cells == n_cells
    return p


def both(spec):
    """(nsx_iso_source for the device, source of the restatement)"""
    from navierstokes_project_nm4pde_amd import nsx
    if spec is None:
        return None, None
    kind, which, component, normal = spec
    return nsx.iso_source(kind, which, component, normal), IR.source(kind, which, component, normal)


def pick_iso(s, q):
    """an isovalue near the q-quantile of the nodal scalars, in the middle of the widest gap between neighbouring values there"""
    v = np.unique(s[np.isfinite(s)])
    k = min(max(int(q * len(v)), 4), len(v) - 5)
    gaps = np.diff(v[k - 4:k + 5])
    j = k - 4 + int(np.argmax(gaps))
    return float(0.5 * (v[j] + v[j + 1]))


def candidates(s, q):
    """pick_iso first; then isovalues that cut off the 1, 2, ... 8 largest / smallest nodal values (cube level 1: its six cells share a diagonal,
    and most level sets cross all of them)"""
    yield pick_iso(s, q)
    v = np.unique(s[np.isfinite(s)])
    for k in range(1, 9):
        yield float(0.5 * (v[-k - 1] + v[-k]))
        yield float(0.5 * (v[k - 1] + v[k]))


def device_nodal(dev):
    dev.compute_nodal_fields()
    return {name: dev.nodal_field(k) for k, name in enumerate(NR.NAMES)}


def compare(test, case, got, ref):
    """counts and cells exactly, vertices and colour within the derived bound; returns the largest error / bound"""
    pts, col, cells = got
    assert len(cells) == len(ref["cells"]), (case, len(cells), len(ref["cells"]))
    assert np.array_equal(cells, ref["cells"]), case
    out = {}
    for name, g, r, bound in (("points", pts, ref["points_ld"], ref["bound_x"]), ("colour", col, ref.get("colour_ld"), ref["bound_c"])):
        if r is None:
            assert g is None
            continue
        d = np.abs(g.astype(np.longdouble) - r).astype(np.float64)
        ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
        out[name] = float(ratio.max()) / EPS6 if ratio.size else 0.0
    print(case, len(cells), {k: "%.3f of the bound" % v for k, v in out.items()})
    record(test, case=case, n_primitives=int(len(cells)), **{k + "_over_bound": v for k, v in out.items()})
    for k, v in out.items():
        assert v <= 1.0, (case, k, v)
    return out


def same_bits(a, b, what=""):
    for x, y in zip(a, b):
        assert (x is None) == (y is None), what
        if x is not None:
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), what


# ---------------------------------------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize("sources", list(SOURCES))
@pytest.mark.parametrize("mesh", list(MESHES))
def test_parity_with_the_restatement(mesh, sources):
    p = problem(mesh)
    u = p.smooth_velocity()
    (fd, fr), (cd, cr) = both(SOURCES[sources][0]), both(SOURCES[sources][1])
    dev = p.device()
    try:
        dev.set_solution(u)
        nodal = device_nodal(dev) if IR.NODAL in (fr["kind"], cr["kind"]) else None
        s = IR.nodal_scalar(p.dofs, u, fr, nodal)
        for iso in candidates(s, 0.7):                                                   # the first isovalue that is no vacuous case, judged on the restatement
            ref = IR.extract(p.dofs, u, fr, iso, colour=cr, nodal=nodal)
            if 0 < len(ref["cells"]) and len(np.unique(ref["cells"])) < p.dofs.n_cells:
                break
        assert np.abs(s - iso).min() > 1e-9 * np.abs(s).max()                            # the precondition, on the restatement
        assert 0 < len(ref["cells"])                                                     # against a vacuous pass
        if (mesh, sources) == ("cube1", "pressure-u1"):
            # The one case in which "fewer than all cells are active" cannot hold for ANY isovalue: the six cells of cube level 1 share the
            # diagonal, and the Ethier-Steinmann pressure of smooth_velocity() is symmetric under the rotation about it: its maximum sits at
            # an end of the diagonal (a node of every cell) and its minimum at three vertices of which every cell holds one, so every cell
            # holds a node below and a node above every value in between.  Fewer than all SUB-SIMPLICES are active instead.
            rows = NR.cell_nodes(p.dofs)
            lows = np.nonzero(s == s.min())[0]
            assert all(int(s.argmax()) in row and any(n in row for n in lows) for row in rows)
            assert len(np.unique(ref["cells"])) == 6 and len(set(zip(ref["cells"], ref["sub"]))) < 8 * 6
        else:
            assert len(np.unique(ref["cells"])) < p.dofs.n_cells
        got = dev.extract_isosurface(fd, iso, cd)
        assert got[0].shape == (len(got[2]), p.dim, p.dim) and got[1].shape == (len(got[2]), p.dim)
        compare("iso_parity", "%s-%s" % (mesh, sources), got, ref)
    finally:
        dev.close()


def test_mirrored_cells_swap_their_last_two_vertices():
    """every cell with det J < 0 (the box mirrored in x): parity with the restatement, whose orientation tests/test_iso_reference.py checks"""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    for dim in (2, 3):
        mesh = Mesh.box(dim, [3, 3, 2][:dim], hi=[1.0, 2.0, 1.5][:dim])
        mesh.vertices[:, 0] = -mesh.vertices[:, 0]
        dofs = DoFs(mesh)
        assert (IR.cell_det(dofs) < 0).all()
        spec = (IR.PLANE, 0, 0, [-1.0, 0.73, 0.45][:dim])
        dev = nsx.Nsx(dofs, Tables(dim), 1e-3, 1e-2)
        try:
            dev.set_solution(np.zeros(dofs.n_dofs))
            ref = IR.extract(dofs, np.zeros(dofs.n_dofs), both(spec)[1], 1.31, colour=both(spec)[1])
            assert len(ref["cells"]) > 0
            compare("iso_mirrored", "box%dd" % dim, dev.extract_isosurface(both(spec)[0], 1.31, both(spec)[0]), ref)
        finally:
            dev.close()


# ---------------------------------------------------------------------------------------------- 2. exact ties
def test_exact_ties_give_the_node_positions_bitwise():
    p = problem("box3d")
    X = NR.node_points(p.dofs)
    u = np.zeros(p.dofs.n_dofs)
    u[0:p.dofs.n_u:3] = np.floor(6.0 * X[:, 0] + 3.0 * X[:, 1])                          # integers 0 .. 12, constant along z
    fd, fr = both((IR.VELOCITY, 0, 0, None))
    dev = p.device()
    try:
        dev.set_solution(u)
        for iso in (3.0, 6.0):
            ref = IR.extract(p.dofs, u, fr, iso)
            assert (ref["s"] == iso).sum() > 10
            pts, _, cells = dev.extract_isosurface(fd, iso)
            assert len(cells) == len(ref["cells"]) > 0 and np.array_equal(cells, ref["cells"])
            tie = ref["t"] == 0.0
            assert tie.sum() > 10
            assert np.array_equal(pts[tie], X[ref["node_a"][tie]])                       # t = 0: the inside node itself, bit by bit
            assert (IR.measure(pts) == 0).any()                                          # zero-area primitives are emitted as they come
            compare("iso_ties", "box3d-iso%g" % iso, (pts, None, cells), ref)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 3. empty and full
def test_empty_result_and_a_plane_through_every_cell():
    import itertools
    p = problem("cube1")
    u = p.smooth_velocity()
    dev = p.device()
    try:
        dev.set_solution(u)
        L, h = dev.L, dev._h
        fd, fr = both((IR.VELOCITY, 0, -1, None))
        s = IR.nodal_scalar(p.dofs, u, fr)
        n = ctypes.c_int64(-1)
        assert L.nsx_extract_isosurface(h, ctypes.byref(fd), float(s.max() + 1.0), None, ctypes.byref(n)) == 0 and n.value == 0
        assert L.nsx_get_isosurface(h, None, None, None) == 0
        pts, col, cells = dev.extract_isosurface(fd, float(s.max() + 1.0))
        assert pts.shape == (0, 3, 3) and col is None and cells.shape == (0,)
        full = None
        for sign in itertools.product((1.0, -1.0), repeat=2):                            # the plane across the diagonal all six cells share
            spec = (IR.PLANE, 0, 0, [1.0, sign[0] * 0.9, sign[1] * 1.1])
            ref = IR.extract(p.dofs, u, both(spec)[1], 0.013)
            if len(np.unique(ref["cells"])) == 6:
                full = (spec, ref)
        assert full is not None
        got = dev.extract_isosurface(both(full[0])[0], 0.013)
        assert len(np.unique(got[2])) == 6
        compare("iso_full", "cube1", got, full[1])
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 4. the branches of the scan
def test_workgroup_widths_agree_bitwise_and_the_scan_loops(monkeypatch):
    p = Problem("box", 3, n=[9, 9, 9])
    assert p.dofs.n_cells == 4374 and -(-4374 // 64) == 69                               # 69 totals at 64 lanes: two passes of the looping level
    u = p.smooth_velocity()
    (fd, fr), (cd, cr) = both((IR.VELOCITY, 0, -1, None)), both((IR.PRESSURE, 0, 0, None))
    s = IR.nodal_scalar(p.dofs, u, fr)
    iso = pick_iso(s, 0.5)
    ref = IR.extract(p.dofs, u, fr, iso, colour=cr)
    assert ref["cells"].max() > 64 * 64                                                  # primitives behind the first pass of the loop
    dev = p.device()
    try:
        dev.set_solution(u)
        results = {}
        for wg in ("64", "256", "128", "7"):                                             # anything else: the default
            monkeypatch.setenv("NSX_ISO_WG", wg)
            results[wg] = dev.extract_isosurface(fd, iso, cd)
        monkeypatch.delenv("NSX_ISO_WG")
        results["unset"] = dev.extract_isosurface(fd, iso, cd)
        for wg in ("64", "128", "7", "unset"):
            same_bits(results[wg], results["256"], wg)
        compare("iso_scan", "box3d-9x9x9", results["64"], ref)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 5. watertightness of the device's output
def test_sphere_from_the_device_is_closed_and_oriented():
    import test_iso_reference as T
    p = Problem("cube", 3, 4)
    u = T.sphere_state(p.dofs)
    fd, fr = both((IR.VELOCITY, 0, 0, None))
    dev = p.device()
    try:
        dev.set_solution(u)
        pts, _, cells = dev.extract_isosurface(fd, T.SPHERE_R2)
        closed, euler = IR.is_closed_oriented(pts)                                       # vertex pairs compared as bytes
        assert len(cells) == 870 and closed and euler == 2
        compare("iso_sphere", "cube4", (pts, None, cells), IR.extract(p.dofs, u, fr, T.SPHERE_R2))
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 6. layout independence
def test_layout_and_rank_tables_change_no_bit():
    from navierstokes_project_nm4pde_amd import nsx
    p = problem("cyl3d")
    p4 = Problem("cylinder", 3, 1, n_sub=4)
    assert np.array_equal(p.mesh.cells, p4.mesh.cells) and np.array_equal(p.mesh.vertices, p4.mesh.vertices)
    u = p.smooth_velocity()
    u4 = np.zeros_like(u)
    u4[np.asarray(p4.dofs.cell_dofs).ravel()] = u[np.asarray(p.dofs.cell_dofs).ravel()]   # the same state, dof by dof
    (sd, sr), (pd, _), (qd, _) = both((IR.VELOCITY, 0, -1, None)), both((IR.PRESSURE, 0, 0, None)), both((IR.NODAL, 2, 0, None))
    iso = pick_iso(IR.nodal_scalar(p.dofs, u, sr), 0.6)

    def run(dev, state):
        try:
            dev.set_solution(state)
            dev.compute_nodal_fields()
            return dev.extract_isosurface(sd, iso, pd) + dev.extract_isosurface(qd, 0.05, sd)
        finally:
            dev.close()
    plain = run(p.device(), u)
    assert len(plain[2]) > 100 and len(plain[5]) > 100
    same_bits(run(p4.device(), u4), plain, "rank tables")
    for layout in ((8, nsx.FIRST_TOUCH, 0), (4, nsx.COLOUR, 0), (64, nsx.COLOUR, 0)):
        dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=layout)
        assert dev.layout_info()["on"] and dev.layout_info()["ranks"] == layout[0]
        same_bits(run(dev, u), plain, str(layout))
    # a layout switched on a handle that has extracted already: the node maps follow
    dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat)
    try:
        dev.set_solution(u)
        dev.compute_nodal_fields()
        same_bits(dev.extract_isosurface(qd, 0.05, sd), plain[3:], "before the switch")
        dev.set_internal_layout(8, nsx.COLOUR, 0)
        same_bits(run(dev, u), plain, "behind the switch")
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 7. purity and reproducibility
def test_the_call_changes_no_state_and_two_calls_agree_bitwise():
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    p = Problem("cylinder", 2, 1)
    u = p.smooth_velocity()
    (sd, sr), (pd, _) = both((IR.VELOCITY, 0, -1, None)), both((IR.PRESSURE, 0, 0, None))
    iso = pick_iso(IR.nodal_scalar(p.dofs, u, sr), 0.5)
    dev, twin = p.device(), p.device()
    try:
        for h in (dev, twin):
            h.set_solution(u)
            h.assemble(nsx.TEMAM)
            h.apply_boundary_values(*cylinder_boundary_values(p.dofs, InletVelocity(2, 3), p.deltat))
        first = dev.extract_isosurface(sd, iso, pd)                                      # between the boundary values and the solve
        assert len(first[2]) > 10
        same_bits(dev.extract_isosurface(sd, iso, pd), first, "second call")
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.rhs, twin.rhs)
        sa, sb = dev.solve_time_step(nsx.YOSIDA), twin.solve_time_step(nsx.YOSIDA)
        for key in ("outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves", "status", "final_residual"):
            assert sa[key] == sb[key], key
        assert np.array_equal(dev.solution, twin.solution) and np.array_equal(dev.solution_owned, twin.solution_owned)
        assert np.array_equal(dev.rhs, twin.rhs)
        kept = (np.empty_like(first[0]), np.empty_like(first[1]), np.empty_like(first[2]))
        assert dev.L.nsx_get_isosurface(dev._h, kept[0].ctypes.data_as(_f64p), kept[1].ctypes.data_as(_f64p), kept[2].ctypes.data_as(_i32p)) == 0
        same_bits(kept, first, "no recompute behind the solve")
        moved = dev.extract_isosurface(sd, iso, pd)
        assert moved[0].tobytes() != first[0].tobytes()                                  # the solved state gives another curve
    finally:
        dev.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 8. not finite
def test_a_nan_removes_exactly_the_sub_simplices_that_hold_the_node():
    p = problem("cyl3d")
    cd, cn = np.asarray(p.dofs.cell_dofs), NR.cell_nodes(p.dofs)
    u = p.smooth_velocity()
    (fd, fr), (cdv, cr) = both((IR.VELOCITY, 0, 1, None)), both((IR.PRESSURE, 0, 0, None))
    s = IR.nodal_scalar(p.dofs, u, fr)
    iso = pick_iso(s, 0.5)
    clean_ref = IR.extract(p.dofs, u, fr, iso, colour=cr)
    # a node of a sub-simplex that the surface crosses, so that primitives do disappear
    k = len(clean_ref["cells"]) // 2
    node = int(clean_ref["node_a"][k, 0])
    bad = u.copy()
    bad[3 * node + 1] = float("nan")
    subs = np.array(IR.SUB[3])
    holds = (cn[clean_ref["cells"][:, None], subs[clean_ref["sub"]]] == node).any(axis=1)
    assert 0 < holds.sum() < len(holds) // 4
    dev = p.device()
    try:
        dev.set_solution(u)
        clean = dev.extract_isosurface(fd, iso, cdv)
        assert len(clean[2]) == len(holds)
        dev.set_solution(bad)
        n = ctypes.c_int64(-1)
        assert dev.L.nsx_extract_isosurface(dev._h, ctypes.byref(fd), iso, ctypes.byref(cdv), ctypes.byref(n)) == 0      # the call succeeds
        assert n.value == (~holds).sum()
        got = dev.extract_isosurface(fd, iso, cdv)
        same_bits(got, tuple(a[~holds] for a in clean), "everything else")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 9. argument errors
def test_argument_errors():
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    S = nsx.iso_source
    n = ctypes.c_int64(-5)
    speed = S(nsx.ISO_VELOCITY, component=-1)
    ARG, UNSUPPORTED = -1, -3
    dev = p.device()
    try:
        L, h = dev.L, dev._h

        def ext(field, iso=0.5, colour=None, count=n):
            return L.nsx_extract_isosurface(h, ctypes.byref(field) if field is not None else None, float(iso),
                                            ctypes.byref(colour) if colour is not None else None, ctypes.byref(count) if count is not None else None)
        assert L.nsx_get_isosurface(h, None, None, None) == ARG                          # no extract on this mesh yet
        assert b"nsx_get_isosurface" in L.nsx_last_error(h) and b"nsx_extract_isosurface first" in L.nsx_last_error(h)
        assert L.nsx_extract_isosurface(None, ctypes.byref(speed), 0.5, None, ctypes.byref(n)) == ARG and L.nsx_get_isosurface(None, None, None, None) == ARG
        dev.set_solution(p.smooth_velocity())
        assert ext(S(nsx.ISO_NODAL, which=nsx.FIELD_Q)) == ARG                           # no nodal results on this mesh
        assert b"nsx_compute_nodal_fields" in L.nsx_last_error(h)
        good = dev.extract_isosurface(speed, 0.2, S(nsx.ISO_PRESSURE))
        assert len(good[2]) > 10
        refused = [
            ext(None), ext(speed, count=None),
            ext(S(4)), ext(S(-1)), ext(speed, colour=S(17)),                                                  # kind
            ext(S(nsx.ISO_VELOCITY, component=2)), ext(S(nsx.ISO_VELOCITY, component=-2)),                    # component
            ext(S(nsx.ISO_NODAL, which=nsx.FIELD_COUNT)), ext(S(nsx.ISO_NODAL, which=-1)),                    # which
            ext(speed, iso=float("nan")), ext(speed, iso=float("inf")),
            ext(S(nsx.ISO_PLANE, normal=[0.0, 0.0])), ext(S(nsx.ISO_PLANE, normal=[1.0, float("nan")])),
            ext(S(nsx.ISO_PLANE, normal=[float("inf"), 1.0])), ext(speed, colour=S(nsx.ISO_PLANE, normal=[0.0, 0.0])),
        ]
        assert refused == [ARG] * len(refused), refused
        assert b"nsx_extract_isosurface" in L.nsx_last_error(h)
        dev.compute_nodal_fields()
        assert ext(S(nsx.ISO_NODAL, which=nsx.FIELD_VORTICITY, component=1)) == ARG      # one component in 2D
        assert ext(S(nsx.ISO_NODAL, which=nsx.FIELD_GRADIENT, component=4)) == ARG
        assert ext(S(nsx.ISO_PLANE, normal=[0.0, 1.0, float("nan")]), iso=0.2) == 0      # 2D reads two entries of the normal
        assert n.value > 0
        good = dev.extract_isosurface(speed, 0.2)
        pts = np.empty_like(good[0])
        assert L.nsx_get_isosurface(h, pts.ctypes.data_as(_f64p), pts.ctypes.data_as(_f64p), None) == ARG    # that extract had no colour
        n.value = -5
        assert ext(S(9)) == ARG and n.value == -5                                        # a refused call writes nothing ...
        kept = (np.empty_like(good[0]), None, np.empty_like(good[2]))
        assert L.nsx_get_isosurface(h, kept[0].ctypes.data_as(_f64p), None, kept[2].ctypes.data_as(_i32p)) == 0
        same_bits(kept, good, "... and leaves the earlier result readable")
        # a second nsx_set_mesh drops the result
        cd = np.ascontiguousarray(p.dofs.cell_dofs, dtype=np.int32)
        cc = np.ascontiguousarray(p.dofs.cell_coords, dtype=np.float64)
        assert L.nsx_set_mesh(h, p.dofs.n_cells, p.dofs.dofs_per_cell, cd.ctypes.data_as(_i32p), cc.ctypes.data_as(_f64p), p.dofs.n_u, p.dofs.n_p) == 0
        assert L.nsx_get_isosurface(h, None, None, None) == ARG
        dev.set_solution(p.smooth_velocity())
        same_bits(dev.extract_isosurface(speed, 0.2), good, "the same mesh and state again")
    finally:
        dev.close()
    # handles without tables, mesh or state (raw calls, as tests/test_abi.py makes them)
    L = nsx.lib()
    h = ctypes.c_void_p()
    prm = nsx.Params(2, 0, 1e-3, 1e-2)
    assert L.nsx_create(ctypes.byref(prm), ctypes.byref(h)) == 0
    try:
        assert L.nsx_extract_isosurface(h, ctypes.byref(speed), 0.5, None, ctypes.byref(n)) == ARG           # neither tables nor mesh
        assert b"nsx_set_mesh" in L.nsx_last_error(h)
        t = p.tables
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.N2, t.dN2, t.N1, t.weights)]
        # a (dim, n_p2) other than (2, 6) / (3, 10) never gets as far as a mesh: nsx_set_tables refuses it with NSX_ERR_UNSUPPORTED, and the
        # extraction's own check of the pair (NSX_ERR_UNSUPPORTED as well) stands behind that one
        assert L.nsx_set_tables(h, t.n_q, 10, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == UNSUPPORTED
        assert L.nsx_set_tables(h, t.n_q, t.n_p2, t.n_p1, *[a.ctypes.data_as(_f64p) for a in arrs]) == 0
        assert L.nsx_extract_isosurface(h, ctypes.byref(speed), 0.5, None, ctypes.byref(n)) == ARG           # tables, no mesh
        assert L.nsx_get_isosurface(h, None, None, None) == ARG
    finally:
        L.nsx_destroy(h)


def test_a_one_rank_communicator_is_one_process():
    """NSX_ISO_NODAL is refused across processes only: behind nsx_comm_init with world = 1 it gives the result it gave before"""
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    q, speed = nsx.iso_source(nsx.ISO_NODAL, which=nsx.FIELD_Q), nsx.iso_source(nsx.ISO_VELOCITY, component=-1)
    dev = p.device()
    try:
        dev.set_solution(p.smooth_velocity())
        dev.compute_nodal_fields()
        before = dev.extract_isosurface(q, 0.0, speed)
        assert len(before[2]) > 10
        dev.comm_init_single()
        same_bits(dev.extract_isosurface(q, 0.0, speed), before, "behind the communicator")
        same_bits(dev.extract_isosurface(speed, 0.2, q)[2:], dev.extract_isosurface(speed, 0.2)[2:], "as colour")
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------- 10. distributed
def test_distributed_extraction_is_the_single_process_surface_cell_by_cell(tmp_path):
    """3D cylinder level 1 on 2 processes (one card, gloo, host callbacks) with 2 sub-ranks each, the launch recipe of
    tests/test_gpu_nodal_fields.py on a master port of its own."""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    import iso_dist_worker as W
    dim, level, world, n_sub = 3, 1, 2, 2
    prefix = str(tmp_path / "iso")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29615", os.path.join(ROOT, "tests", "iso_dist_worker.py"), str(dim), str(level), str(n_sub), prefix]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [np.load("%s_rank%d.npz" % (prefix, k)) for k in range(world)]
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh), Tables(dim)
    u = W.state(dofs)
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4)
    try:
        dev.set_solution(u)
        one = {name: dev.extract_isosurface(field, W.isovalue(name, iso, dofs, u), colour) for name, field, iso, colour in W.cases(nsx)}
    finally:
        dev.close()
    for name, (pts, col, cells) in one.items():
        assert len(cells) > 50, name
        seen = np.zeros(dofs.n_cells, dtype=int)
        total = 0
        for k, d in enumerate(ranks):
            gc = d["cell_ids"][d[name + "_cells"]]                                       # the rank's own cell list -> global cells
            assert np.all(np.diff(d[name + "_cells"]) >= 0)
            seen[np.unique(gc)] += 1
            total += len(gc)
            for c in np.unique(gc):                                                      # per global cell: the single handle's primitives, bit by bit
                mine, theirs = gc == c, cells == c
                assert d[name + "_points"][mine].tobytes() == pts[theirs].tobytes(), (name, k, c)
                if col is not None:
                    assert d[name + "_colour"][mine].tobytes() == col[theirs].tobytes(), (name, k, c)
        assert seen.max() == 1 and total == len(cells), name                             # no cell on two ranks, and together all of them
        assert np.array_equal(np.nonzero(seen)[0], np.unique(cells)), name
    for d in ranks:
        before, mid, after = d["counters"]
        assert tuple(before) == tuple(mid) == tuple(after)                               # no collective, no ghost exchange
        assert d["nodal_rc"].tolist() == [-3, -3, -3, 0] and d["n_after_refusal"] == -7   # NSX_ERR_UNSUPPORTED; nothing written
        assert d["kept"].tobytes() == d["pressure_points"].tobytes()                     # the earlier result stayed readable
