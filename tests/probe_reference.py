"""Extended-precision restatement of the point probes (include/nsx.h: nsx_set_probes / nsx_get_probe_cells / nsx_eval_probes), in the manner
of tests/diagnostics_reference.py: barycentric coordinates by Cramer's rule (adjugate over determinant, diagnostics_reference.geometry) in
np.longdouble straight from the vertices, shape functions and sums in np.longdouble.  tests/test_probe_reference.py pins it against the
front-end's pressure_difference, closed forms and a combinatorial tie rule; the GPU tests compare the kernels with it."""
import numpy as np

import diagnostics_reference as R

LD = np.longdouble
TOL = 1e-12                                   # the library's own containment tolerance
LINES = {2: [(0, 1), (1, 2), (2, 0)], 3: [(0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3)]}   # the front-end's local line order


def barycentric(mesh, points, chunk=64):
    """lambda [n_points][n_cells][dim+1] of every point in every cell, long double: x = X0 + J lambda[1:], lambda[0] = 1 - sum"""
    Ji, _ = R.geometry(mesh)
    X0 = np.asarray(mesh.vertices, dtype=LD)[np.asarray(mesh.cells)[:, 0]]          # [nc, dim]
    P = np.asarray(points, dtype=np.float64).reshape(-1, mesh.dim).astype(LD)
    for s in range(0, len(P), chunk):
        r = P[s:s + chunk, None, :] - X0[None, :, :]                                # [np, nc, dim]
        xi = (Ji[None, :, :, :] * r[:, :, None, :]).sum(axis=3)                     # [np, nc, k]
        yield s, np.concatenate([1 - xi.sum(axis=2, keepdims=True), xi], axis=2)


def locate(mesh, points, tol=TOL):
    """cells [n] (lowest containing cell, -1: none), lam [n][dim+1] in that cell (long double, 0 where none), mult [n] containing cells,
    lam_min [n] smallest barycentric coordinate in the chosen cell (-inf where none)"""
    tol = TOL if tol < 0 else tol
    n = len(np.asarray(points).reshape(-1, mesh.dim))
    cells, mult = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    lam = np.zeros((n, mesh.dim + 1), dtype=LD)
    for s, L in barycentric(mesh, points):
        inside = (L >= -LD(tol)).all(axis=2)                                         # a NaN coordinate is in no cell
        for k in range(L.shape[0]):
            hit = np.flatnonzero(inside[k])
            mult[s + k] = len(hit)
            if len(hit):
                cells[s + k] = hit[0]
                lam[s + k] = L[k, hit[0]]
    lam_min = np.where(cells >= 0, lam.min(axis=1).astype(np.float64), -np.inf)
    return cells, lam, mult, lam_min


def shape_p2(lam):
    """N [n][n_p2] and dN [n][n_p2][dim] (derivatives by the reference coordinates xi_k = lambda_k, k = 1..dim) at lam [n][dim+1]"""
    n, nv = lam.shape
    dim = nv - 1
    lines = LINES[dim]
    N = np.zeros((n, nv + len(lines)), dtype=LD)
    g = np.zeros((n, nv + len(lines), nv), dtype=LD)                                 # dN_a / d lambda_m
    for a in range(nv):
        N[:, a] = lam[:, a] * (2 * lam[:, a] - 1)
        g[:, a, a] = 4 * lam[:, a] - 1
    for e, (i, j) in enumerate(lines):
        N[:, nv + e] = 4 * lam[:, i] * lam[:, j]
        g[:, nv + e, i] = 4 * lam[:, j]
        g[:, nv + e, j] = 4 * lam[:, i]
    return N, g[:, :, 1:] - g[:, :, :1]


def evaluate(mesh, dofs, solution, points, tol=TOL):
    """dict of float64 arrays over the points: cells, found, velocity [n][dim], pressure [n], gradient [n][dim][dim] (d_j u_i, in the chosen
    cell), mult, lam_min, lam [n][dim+1] and the absolute-term sums S_u [n][dim] = sum_a |N_a| |U_a,i|, S_p [n] = sum_v |lambda_v| |P_v|,
    S_g [n][dim][dim] = sum_a |U_a,i| |(grad N_a)_j| (grad: the physical gradient J^-T grad_xi N_a).  Not found: everything 0."""
    dim = mesh.dim
    cells, lam, mult, lam_min = locate(mesh, points, tol)
    n = len(cells)
    found = cells >= 0
    c = np.where(found, cells, 0)
    Ji, _ = R.geometry(mesh)
    U = R.cell_velocities(dofs, solution)[c]                                         # [n, np2, dim]
    cd = np.asarray(dofs.cell_dofs)[c]
    P = np.asarray(solution, dtype=np.float64)[cd[:, [(dim + 1) * v + dim for v in range(dim + 1)]]].astype(LD)
    N, dN = shape_p2(lam)
    gN = (dN[:, :, :, None] * Ji[c][:, None, :, :]).sum(axis=2)                      # [n, a, j] physical gradient of N_a
    out = {
        "velocity": (N[:, :, None] * U).sum(axis=1), "S_u": (np.abs(N)[:, :, None] * np.abs(U)).sum(axis=1),
        "pressure": (lam * P).sum(axis=1), "S_p": (np.abs(lam) * np.abs(P)).sum(axis=1),
        "gradient": (U[:, :, :, None] * gN[:, :, None, :]).sum(axis=1), "S_g": (np.abs(U)[:, :, :, None] * np.abs(gN)[:, :, None, :]).sum(axis=1),
    }
    for k, v in out.items():
        v[~found] = 0
        out[k] = v.astype(np.float64)
    lam[~found] = 0
    out.update(cells=cells, found=found, mult=mult, lam_min=lam_min, lam=lam.astype(np.float64))
    return out


def linear_pressure(dofs, g=(2.0, -1.0, 0.5), p0=7.0):
    """p = p0 + g . x at the P1 nodes, as the pressure part of a solution vector (velocity untouched: 0)"""
    v = np.zeros(dofs.n_dofs)
    v[dofs.n_u:] = p0 + np.asarray(dofs.support_points)[dofs.n_u:] @ np.asarray(g[:dofs.dim])
    return v


def quadratic_state(dofs, g=(2.0, -1.0, 0.5), p0=7.0):
    """the quadratic velocity of diagnostics_reference plus a linear pressure: both are their own interpolants"""
    return R.interpolate_quadratic(dofs) + linear_pressure(dofs, g, p0)


def box_points(mesh, n, seed=7, shrink=0.0):
    """n uniform points in the bounding box of the mesh (shrunk towards its centre by the fraction `shrink`), default_rng(seed)"""
    V = np.asarray(mesh.vertices)
    lo, hi = V.min(axis=0), V.max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * (1 - shrink)
    return mid + half * (2 * np.random.default_rng(seed).random((n, mesh.dim)) - 1)


def support_points(dofs, n, seed=11):
    """n distinct P2 support points (vertices and edge mid-points: every one of them lies in several cells)"""
    X = np.asarray(dofs.support_points)[:dofs.n_u:dofs.dim]
    idx = np.random.default_rng(seed).choice(len(X), size=min(n, len(X)), replace=False)
    return X[np.sort(idx)].copy()


def pressure_points(dim):
    return np.array([[0.45, 0.2, 0.205], [0.55, 0.2, 0.205]]) if dim == 3 else np.array([[0.15, 0.2], [0.25, 0.2]])


def outside_points(dim):
    """three points outside the bounding box of the cylinder meshes and one in the cylinder's hole (centre (0.5, 0.2) in 3D, (0.2, 0.2) in 2D,
    radius 0.05)"""
    if dim == 3:
        return np.array([[9.0, 9.0, 9.0], [-1.0, 0.2, 0.2], [1.0, 0.2, 5.0], [0.5, 0.2, 0.2]])
    return np.array([[9.0, 9.0], [-1.0, 0.2], [1.0, -3.0], [0.2, 0.2]])
