"""CPU suite: tests/probe_reference.py, the extended-precision restatement the GPU tests of the point probes compare the kernels with, pinned
against the front-end's two pressure_difference implementations, against closed forms and against a tie rule worked out combinatorially --
so that those tests do not rest on a restatement alone."""
import numpy as np
import pytest

import diagnostics_reference as R
import probe_reference as PR


def _problem(kind, dim, level=1):
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh
    mesh = Mesh.cylinder(dim, level) if kind == "cylinder" else Mesh.box(dim, [3, 3, 2][:dim], hi=[1.0, 2.0, 1.5][:dim])
    return mesh, DoFs(mesh)


@pytest.mark.parametrize("dim", [2, 3])
def test_p1_value_at_the_pressure_points_is_the_front_ends(dim):
    """the vector of tests/test_frontend.py::test_pressure_difference_is_the_p1_interpolant; the reference's two points and that test's"""
    from navierstokes_project_nm4pde_amd.problem import pressure_difference
    mesh, dofs = _problem("cylinder", dim)
    g = np.array([2.0, -1.0, 0.5][:dim])
    sol = PR.linear_pressure(dofs)
    for a, b in (PR.pressure_points(dim), np.array([[0.45, 0.2, 0.205][:dim], [0.55, 0.2, 0.205][:dim]])):
        ev = PR.evaluate(mesh, dofs, sol, np.array([a, b]))
        assert ev["found"].all()
        diff = ev["pressure"][0] - ev["pressure"][1]
        front, n_found = dofs.pressure_difference(sol, a, b)
        assert n_found == 2
        assert abs(diff - front) < 1e-12 and abs(diff - pressure_difference(mesh, dofs, sol, a, b)) < 1e-12
        assert abs(diff - (a - b) @ g) < 1e-12
    # a point nobody holds contributes 0, as the front-end's
    ev = PR.evaluate(mesh, dofs, sol, np.array([PR.pressure_points(dim)[0], [9.0] * dim]))
    front, n_found = dofs.pressure_difference(sol, PR.pressure_points(dim)[0], np.array([9.0] * dim))
    assert n_found == 1 and ev["found"].tolist() == [True, False] and ev["pressure"][1] == 0.0 and ev["cells"][1] == -1
    assert abs(ev["pressure"][0] - front) < 1e-12


@pytest.mark.parametrize("kind,dim", [("box", 2), ("box", 3), ("cylinder", 2), ("cylinder", 3)])
def test_quadratic_velocity_and_linear_pressure_are_reproduced(kind, dim):
    """a quadratic field is its own P2 interpolant and a linear one its own P1 interpolant: values and gradient at 200 uniform points of the
    bounding box match the polynomials to 1e-14 * scale (scale: the absolute-term sums, at least the largest nodal value)"""
    mesh, dofs = _problem(kind, dim)
    g = np.array([2.0, -1.0, 0.5][:dim])
    sol = PR.quadratic_state(dofs)
    pts = PR.box_points(mesh, 200)
    ev = PR.evaluate(mesh, dofs, sol, pts)
    f = ev["found"]
    assert f.sum() >= (200 if kind == "box" else 180)
    u, G = R.quadratic_field(pts.astype(np.longdouble))
    u, G = u.astype(np.float64), G.astype(np.float64)
    assert np.all(np.abs(ev["velocity"] - u)[f] <= 1e-14 * np.maximum(ev["S_u"], 1.0)[f])
    assert np.all(np.abs(ev["pressure"] - (7.0 + pts @ g))[f] <= 1e-14 * ev["S_p"][f])
    assert np.all(np.abs(ev["gradient"] - G)[f] <= 1e-14 * np.maximum(ev["S_g"], 1.0)[f])
    assert (ev["S_p"][f] >= np.abs(ev["pressure"][f])).all() and (ev["S_u"][f] >= np.abs(ev["velocity"][f]) * (1 - 1e-15)).all()
    # not found: exact zeros
    for k in ("velocity", "pressure", "gradient", "S_u", "S_p", "S_g", "lam"):
        assert not ev[k][~f].any()
    assert (ev["cells"][~f] == -1).all() and (ev["mult"][~f] == 0).all()
    # the barycentric coordinates reproduce the point
    X = np.asarray(mesh.vertices)[np.asarray(mesh.cells)[ev["cells"][f]]]
    assert np.abs(np.einsum("nv,nvd->nd", ev["lam"][f], X) - pts[f]).max() < 1e-14 and np.abs(ev["lam"][f].sum(axis=1) - 1).max() < 1e-15


@pytest.mark.parametrize("kind,dim", [("box", 3), ("cylinder", 2), ("cylinder", 3)])
def test_a_vertex_goes_to_the_lowest_cell_that_has_it(kind, dim):
    """at (up to) 200 mesh vertices the located cell is the lowest cell of mesh.cells that lists the vertex -- found combinatorially, with no
    arithmetic -- and `mult` counts the cells around it"""
    mesh, dofs = _problem(kind, dim)
    cells = np.asarray(mesh.cells)
    nv = len(mesh.vertices)
    ids = np.sort(np.random.default_rng(5).choice(nv, size=min(200, nv), replace=False))
    first = np.full(nv, -1)
    count = np.zeros(nv, dtype=int)
    for c in range(len(cells) - 1, -1, -1):
        first[cells[c]] = c
    np.add.at(count, cells.ravel(), 1)
    got, lam, mult, lam_min = PR.locate(mesh, np.asarray(mesh.vertices)[ids])
    assert np.array_equal(got, first[ids])
    assert np.array_equal(mult, count[ids]) and mult.min() >= 1 and mult.max() > 1
    assert np.abs(lam_min).max() < 1e-14 and np.abs(lam.max(axis=1).astype(float) - 1).max() < 1e-14
