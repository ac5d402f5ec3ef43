"""CPU suite: pins tests/tracer_reference.py, the extended-precision restatement the GPU tests compare k_tracer_advect with -- its
face-neighbour table against the front-end's boundary faces, its walk and its three schemes against closed-form pathlines."""
import numpy as np
import pytest

import probe_reference as PR
import tracer_reference as TR
from conftest import Problem

MESHES = [("box", 2, 1), ("box", 3, 1), ("cube", 3, 1), ("cylinder", 2, 2), ("cylinder", 3, 1)]


def problem(kind, dim, level):
    return Problem(kind, dim, level) if kind != "box" else Problem(kind, dim)


@pytest.mark.parametrize("kind,dim,level", MESHES)
def test_adjacency_is_symmetric_and_its_boundary_is_the_front_ends(kind, dim, level):
    p = problem(kind, dim, level)
    cells = np.asarray(p.mesh.cells)
    nbr = TR.adjacency(cells)
    nv, nc = nbr.shape
    assert (nv, nc) == (dim + 1, len(cells))
    for k in range(nv):
        for c in np.flatnonzero(nbr[k] >= 0):
            d = nbr[k, c]
            back = np.flatnonzero(nbr[:, d] == c)
            assert len(back) == 1 and d != c
            shared = set(cells[c]) - {cells[c, k]}
            assert shared == set(cells[d]) - {cells[d, back[0]]} and len(shared) == dim
    assert (nbr == -1).sum() == len(p.mesh.bfaces)
    front = {(int(c), tuple(sorted(int(v) for v in f))) for c, f in zip(p.mesh.bface_cells, p.mesh.bfaces)}
    table = TR.TETF if dim == 3 else TR.TRIF
    mine = set()
    for k, c in zip(*np.nonzero(nbr == -1)):
        face = TR.exit_face(dim, int(k))
        verts = tuple(sorted(int(cells[c, a]) for a in table[face]))           # deal.II's face number names the same vertices
        assert verts == tuple(sorted(int(v) for a, v in enumerate(cells[c]) if a != k))
        mine.add((int(c), verts))
    assert mine == front


@pytest.mark.parametrize("kind,dim", [("box", 2), ("box", 3)])
@pytest.mark.parametrize("scheme", [TR.EULER, TR.RK2, TR.RK4])
def test_uniform_field_carries_particles_across_cells(kind, dim, scheme):
    p = problem(kind, dim, 1)
    b = np.array([0.25, -0.5, 0.125][:dim])
    state = TR.linear_state(p.dofs, np.zeros((dim, dim)), np.zeros(dim), b)
    pts = PR.box_points(p.mesh, 40, shrink=0.5)
    T = 0.5
    st = TR.run(p.mesh, p.dofs, state, pts, T, 8, scheme)
    assert (st["status"] == TR.ACTIVE).all() and (st["cells"] != PR.locate(p.mesh, pts)[0]).mean() > 0.3 and st["hops"].max() >= 1
    err = np.abs(st["positions_ld"] - (pts.astype(np.longdouble) + np.longdouble(T) * b)).max()
    assert err <= 1e-17 * TR.diagonal(p.mesh) * 8
    assert np.array_equal(st["age"], np.full(len(pts), T))
    found = PR.locate(p.mesh, st["positions"])[0]
    sure = st["margin"] > 1e-9
    assert sure.mean() > 0.9 and np.array_equal(found[sure], st["cells"][sure])   # the walk ends where the search would


@pytest.mark.parametrize("kind,dim", [("box", 2), ("box", 3), ("cube", 3)])
@pytest.mark.parametrize("scheme", [TR.EULER, TR.RK2, TR.RK4])
@pytest.mark.parametrize("dt", [0.5, -0.5])
def test_rigid_rotation_follows_the_schemes_polynomial(kind, dim, scheme, dt):
    p = problem(kind, dim, 1)
    V = np.asarray(p.mesh.vertices)
    c = (V.min(axis=0) + V.max(axis=0)) / 2
    A = TR.rotation_matrix(dim)
    state = TR.linear_state(p.dofs, A, c)
    pts = PR.box_points(p.mesh, 40, shrink=0.4)
    n = 8
    st = TR.run(p.mesh, p.dofs, state, pts, dt, n, scheme)
    assert (st["status"] == TR.ACTIVE).all() and (st["cells"] != PR.locate(p.mesh, pts)[0]).any()
    exact = TR.linear_closed_form(pts, A, c, np.longdouble(dt) / n, n, scheme)
    assert np.abs(st["positions_ld"] - exact).max() <= 1e-16 * TR.diagonal(p.mesh)
    # LINEAR between two multiples of the field: theta enters; with previous = solution it is the frozen field again
    lin = TR.run(p.mesh, p.dofs, state, pts, dt, n, scheme, TR.LINEAR, previous=state)
    assert np.abs(lin["positions_ld"] - exact).max() <= 1e-16 * TR.diagonal(p.mesh)
    half = TR.run(p.mesh, p.dofs, state, pts, dt, n, TR.EULER, TR.LINEAR, previous=np.zeros_like(state))
    # Euler through theta_s u with theta_s = s / n (forward) or 1 - s / n (backward): the product of (I + h theta_s A)
    h = np.longdouble(dt) / n
    x = pts.astype(np.longdouble) - c
    for s in range(n):
        theta = np.longdouble(s) / n if dt > 0 else 1 - np.longdouble(s) / n
        x = x + h * theta * (x @ np.asarray(A, dtype=np.longdouble).T)
    assert np.abs(half["positions_ld"] - (x + c)).max() <= 1e-16 * TR.diagonal(p.mesh)


def test_particles_leave_through_the_face_they_cross_and_stay_where_the_substep_began():
    p = problem("box", 2, 1)                                                     # [0, 1] x [0, 2]
    state = TR.linear_state(p.dofs, np.zeros((2, 2)), np.zeros(2), np.array([1.0, 0.0]))
    pts = np.array([[0.3, 0.7], [0.9, 1.3], [5.0, 5.0]])
    st = TR.run(p.mesh, p.dofs, state, pts, 0.5, 4, TR.RK4)
    assert st["status"].tolist() == [TR.ACTIVE, TR.EXITED, TR.NOT_FOUND]
    assert np.allclose(st["positions"][0], [0.8, 0.7]) and st["age"][0] == 0.5
    assert np.allclose(st["positions"][1], [0.9, 1.3]) and st["age"][1] == 0.0  # 0.9 + 0.125 leaves in the first substep
    c, face = int(st["cells"][1]), int(st["exit_faces"][1])
    verts = np.asarray(p.mesh.vertices)[np.asarray(p.mesh.cells)[c][list(TR.TRIF[face])]]
    assert np.array_equal(verts[:, 0], [1.0, 1.0])                              # the exit face lies on x = 1
    assert st["cells"][2] == -1 and st["exit_faces"][2] == -1 and np.array_equal(st["positions"][2], pts[2]) and st["exit_faces"][0] == -1
    # a state value that is not finite: the particles that meet it are LOST, the others go on
    bad = state.copy()
    X = np.asarray(p.dofs.support_points)
    bad[:p.dofs.n_u][X[:p.dofs.n_u, 0] > 0.9] = np.nan                          # the nodes on x = 1: every cell right of x = 2/3 holds one
    lost = TR.run(p.mesh, p.dofs, bad, np.array([[0.3, 0.7], [0.05, 0.7]]), 0.5, 4, TR.RK4)
    assert lost["status"].tolist() == [TR.LOST, TR.ACTIVE] and lost["exit_faces"][0] == -1
    # the third substep starts at x = 0.55 and its last stage point, 0.675, is the first to meet a NaN
    assert lost["age"].tolist() == [0.25, 0.5] and np.allclose(lost["positions"][0], [0.55, 0.7]) and lost["cells"][0] >= 0
