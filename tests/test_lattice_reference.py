"""CPU suite: tests/lattice_reference.py (the restatement the GPU tests of the lattice sampling compare the kernels with) against closed
forms (to 1e-14 * scale, the scale of tests/test_probe_reference.py: the absolute-term sums, at least 1) -- the pinned coordinate formula
and the order of the points, probe_reference.quadratic_state (reproduced exactly by P2/P1), a quadratic nodal field -- its rasterised
search against probe_reference's search of every cell, and the lattices of tests/test_gpu_lattice.py against vacuous passes, so that they
are known to test something before a GPU is used."""
import numpy as np
import pytest

import diagnostics_reference as R
import lattice_reference as LR
import probe_reference as PR
from conftest import Problem

_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(*LR.problem_of(name))
    return _problems[name]


def test_points_follow_the_pinned_formula_x_fastest():
    origin, spacing, counts = (0.1, -0.7, 1e6), (0.1, 1.0 / 3.0, 1e-7), (4, 3, 5)
    pts = LR.points(origin, spacing, counts)
    assert pts.shape == (60, 3)
    for lin in range(60):
        i = (lin % 4, lin // 4 % 3, lin // 12)
        for d in range(3):
            assert pts[lin, d] == origin[d] + float(i[d]) * spacing[d]              # Python floats: one rounded product, one rounded sum
    # an axis of one point, and the lattice over a bounding box
    p = problem("box3")
    o, s = LR.span(p.mesh, (5, 1, 4))
    assert np.array_equal(o, [0.0, 1.0, 0.0]) and np.array_equal(s, [0.25, 1.0, 0.5])
    o, s = LR.span(p.mesh, (5, 3, 4), 0.5)
    assert np.allclose(o, [-0.5, -1.0, -0.75]) and np.allclose(o + s * (np.array([5, 3, 4]) - 1), [1.5, 3.0, 2.25])


@pytest.mark.parametrize("name", ["box2", "box3", "cube"])
def test_quadratic_state_and_quadratic_nodal_field_are_reproduced(name):
    p = problem(name)
    dim = p.dim
    counts = (9, 7, 5)[:dim]
    origin, spacing = LR.span(p.mesh, counts, -0.03)                                 # interior points
    state = PR.quadratic_state(p.dofs)
    for raster in (False, True):
        ref = LR.evaluate(p.mesh, p.dofs, state, origin, spacing, counts, raster=raster)
        pts = LR.points(origin, spacing, counts)
        assert ref["found"].all()
        u, G = R.quadratic_field(pts.astype(np.longdouble))
        assert (np.abs(ref["velocity"] - u.astype(np.float64)) <= 1e-14 * np.maximum(ref["S_u"], 1.0)).all()
        assert (np.abs(ref["pressure"] - (7.0 + pts @ np.array([2.0, -1.0, 0.5][:dim]))) <= 1e-14 * ref["S_p"]).all()
        assert (np.abs(ref["gradient"] - G.astype(np.float64)) <= 1e-14 * np.maximum(ref["S_g"], 1.0)).all()
    V, q = LR.quadratic_nodal(p.dofs)
    val, S = LR.interpolate_nodal(p.mesh, p.dofs, V, pts, ref["cells"])
    assert val.shape == (len(pts), 3) and (S >= np.abs(val) * (1 - 1e-15)).all() and (S[:, 0] > 0).all()
    assert (np.abs(val - q(pts)) <= 1e-14 * np.maximum(S, 1.0)).all()
    # outside: exact zeros
    cells = ref["cells"].copy()
    cells[::2] = -1
    val, S = LR.interpolate_nodal(p.mesh, p.dofs, V, pts, cells)
    assert not val[::2].any() and not S[::2].any() and val[1::2].any()


@pytest.mark.parametrize("name,counts,over,tol", [("cyl2", (40, 12), 0.15, -1.0), ("cyl2", (40, 12), 0.15, 0.05), ("cyl2", (40, 12), 0.15, 0.0),
                                                  ("cyl2", (33, 9), 0.0, 0.5), ("box3", (7, 7, 5), 0.1, -1.0), ("box3", (5, 4, 3), 0.2, 0.05)])
def test_rasterised_search_is_the_search_of_every_cell(name, counts, over, tol):
    p = problem(name)
    origin, spacing = LR.span(p.mesh, counts, over)
    full = PR.locate(p.mesh, LR.points(origin, spacing, counts), tol)
    fast = LR.locate_raster(p.mesh, origin, spacing, counts, tol)
    for a, b in zip(full, fast):
        assert np.array_equal(a, b)
    assert 0 < (full[0] >= 0).sum() < len(full[0])
    if tol > 0 or name == "box3":                                                    # ties: dilated cells overlap; the box lattices hit faces
        assert (full[2] > 1).any()


def test_the_lattices_of_the_gpu_tests_test_something():
    found = {}
    for name, case in LR.owner_cases().items():
        p = problem(case[0])
        origin, spacing, counts, tol = LR.lattice_of(p.mesh, case)
        assert int(np.prod(counts)) <= 65536, name
        cells, _, mult, _ = LR.locate_raster(p.mesh, origin, spacing, counts, tol)
        found[name] = (cells, mult)
    n = {k: int((c >= 0).sum()) for k, (c, _) in found.items()}
    assert n["box2-255x255"] >= 255 * 255 - 2 * 255 and problem("box2").dofs.n_cells == 18   # 18 cells: thousands of points per box
    for k in ("box2-63x5", "box2-64x5", "box2-65x5"):
        assert n[k] >= len(found[k][0]) - 10
    cells, _ = found["cyl3-5x4x3"]
    assert n["cyl3-5x4x3"] >= 55 and len(np.unique(cells[cells >= 0])) < 0.03 * problem("cyl3").dofs.n_cells   # most cells cover no point
    # the overhanging lattice: points on every side of the mesh and in the hole are in no cell
    p = problem("cyl2")
    origin, spacing, counts, _ = LR.lattice_of(p.mesh, LR.owner_cases()["cyl2-256x64-over"])
    pts = LR.points(origin, spacing, counts)
    cells, _ = found["cyl2-256x64-over"]
    V = np.asarray(p.mesh.vertices)
    for d in range(2):
        assert (pts[:, d] < V[:, d].min()).any() and (pts[:, d] > V[:, d].max()).any()
    hole = np.hypot(pts[:, 0] - 0.2, pts[:, 1] - 0.2) < 0.04
    assert hole.sum() > 50 and (cells[hole] < 0).all()
    assert 0.4 * len(pts) < n["cyl2-256x64-over"] < 0.7 * len(pts)
    # a dilated acceptance takes points the vertex boxes do not hold; tol = 0 loses points of the library's tolerance
    assert n["cyl2-256x64-over-tol0.05"] > n["cyl2-256x64-over"] + 100 and n["cyl2-256x64-over-tol0"] <= n["cyl2-256x64-over"]
    assert n["cube-1x1x1"] == 1 and n["box3-40x1x30"] >= 1200 - 140 and n["box3-outside"] == 0
    cells, mult = found["box2-aligned"]
    assert (cells >= 0).all() and (mult > 1).mean() > 0.5                           # every point a node of the mesh: ties


def test_the_large_lattice_of_the_gpu_tests_finds_56_percent():
    """cylinder 3D level 1, 96 x 64 x 48 over the bounding box enlarged by 10 %: 165160 of 294912 points lie in a cell, the fraction the GPU
    test asserts to lie in [0.3, 1]"""
    p = problem("cyl3")
    counts = (96, 64, 48)
    origin, spacing = LR.span(p.mesh, counts, 0.1)
    cells, _, mult, _ = LR.locate_raster(p.mesh, origin, spacing, counts)
    frac = (cells >= 0).mean()
    print("owned fraction", frac, "ties", (mult > 1).mean())
    assert 0.3 <= frac <= 1.0 and (cells >= 0).sum() == 165160
