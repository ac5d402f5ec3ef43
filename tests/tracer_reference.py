"""Extended-precision restatement of the tracer particles (include/nsx.h: nsx_set_tracers / nsx_advect_tracers / nsx_get_tracers), on top of
tests/diagnostics_reference.py (geometry, nodal velocities) and tests/probe_reference.py (the search, the P2 shape functions): the
face-neighbour table from mesh.cells, the walk rule, the three schemes and both fields, everything in np.longdouble.
tests/test_tracer_reference.py pins it against the front-end's boundary faces and closed forms; the GPU tests compare the kernel with it."""
import numpy as np

import diagnostics_reference as R
import probe_reference as PR

LD = np.longdouble
EULER, RK2, RK4 = 1, 2, 4                                  # NSX_TRACER_*: scheme
FROZEN, LINEAR = 0, 1                                      # field
NOT_FOUND, ACTIVE, EXITED, LOST = 0, 1, 2, 3               # status
MAX_HOPS = 1024
TETF = [(0, 1, 2), (1, 0, 3), (0, 2, 3), (2, 1, 3)]        # deal.II's face -> vertex tables (host/NavierStokes.hpp)
TRIF = [(0, 1), (1, 2), (2, 0)]


def adjacency(cells):
    """nbr [nv][n_cells]: the cell across the face opposite local vertex k, -1 on the boundary.  ValueError for a face with more than two
    cells."""
    cells = np.asarray(cells, dtype=np.int64)
    nc, nv = cells.shape
    faces = {}
    for c in range(nc):
        for k in range(nv):
            faces.setdefault(tuple(sorted(int(v) for a, v in enumerate(cells[c]) if a != k)), []).append((c, k))
    nbr = np.full((nv, nc), -1, dtype=np.int64)
    for key, owners in faces.items():
        if len(owners) > 2 or (len(owners) == 2 and owners[0][0] == owners[1][0]):
            raise ValueError("face %s belongs to %d cells" % (key, len(owners)))
        if len(owners) == 2:
            (c0, k0), (c1, k1) = owners
            nbr[k0, c0], nbr[k1, c1] = c1, c0
    return nbr


def exit_face(dim, k):
    """deal.II local number of the face opposite local vertex k"""
    return 3 - k if dim == 3 else (k + 1) % 3


class Field:
    """what one advect call reads: geometry, neighbours and the nodal velocities of `solution` (and `previous`), long double"""

    def __init__(self, mesh, dofs, solution, previous=None, nbr=None):
        self.dim = mesh.dim
        self.Ji, _ = R.geometry(mesh)
        self.X0 = np.asarray(mesh.vertices, dtype=LD)[np.asarray(mesh.cells)[:, 0]]
        self.nbr = adjacency(mesh.cells) if nbr is None else nbr
        self.U = R.cell_velocities(dofs, solution)
        self.Up = None if previous is None else R.cell_velocities(dofs, previous)

    def lam(self, cell, x):
        xi = self.Ji[cell] @ (x - self.X0[cell])
        return np.concatenate([[1 - xi.sum()], xi])

    def velocity(self, cell, lam, theta=None):
        """u_h at lam in `cell`; theta None: FROZEN (`solution` alone), else u_prev + theta (u - u_prev)"""
        N = PR.shape_p2(lam[None, :])[0][0]
        u = N @ self.U[cell]
        if theta is None:
            return u
        up = N @ self.Up[cell]
        return up + theta * (u - up)


def walk(f, x, cell, tol, stats):
    """(status, cell, lam, k): status 0 = accepted in `cell`; EXITED through the face opposite vertex k of `cell`; LOST"""
    if not np.isfinite(x.astype(np.float64)).all():
        return LOST, cell, None, -1
    for hop in range(MAX_HOPS + 1):
        lam = f.lam(cell, x)
        stats["margin"] = min(stats["margin"], float(np.abs(lam + tol).min()))
        stats["hops"] = max(stats["hops"], hop)
        if (lam >= -tol).all():
            return 0, cell, lam, -1
        k = int(np.argmin(lam))                            # the first of equal minima: the lowest k
        nxt = int(f.nbr[k, cell])
        if nxt < 0:
            return EXITED, cell, None, k
        cell = nxt
    return LOST, cell, None, -1


NODES = {EULER: [0.0], RK2: [0.0, 0.5], RK4: [0.0, 0.5, 0.5, 1.0]}


def advect(f, state, dt, n_substeps, scheme, field, tol=PR.TOL):
    """advance `state` (dict: positions [n][dim] long double, cells, status, exit_faces, age (long double), margin, hops) in place"""
    tol = LD(PR.TOL if tol < 0 else tol)
    h = LD(dt) / LD(n_substeps)
    fwd = dt > 0
    assert field == FROZEN or f.Up is not None
    nodes = NODES[scheme]
    for p in range(len(state["status"])):
        if state["status"][p] != ACTIVE:
            continue
        x, cell, age = state["positions"][p].copy(), int(state["cells"][p]), state["age"][p]
        stats = {"margin": state["margin"][p], "hops": state["hops"][p]}
        for s in range(n_substeps):
            cur, ks, y, st, k = cell, [], x.copy(), 0, -1
            for i, c in enumerate(nodes):
                st, cur, lam, k = walk(f, y, cur, tol, stats)
                if st:
                    break
                theta = (LD(s) + LD(c)) / LD(n_substeps)
                theta = theta if fwd else 1 - theta
                ks.append(f.velocity(cur, lam, theta if field == LINEAR else None))
                if i + 1 < len(nodes):
                    y = x + h * LD(nodes[i + 1]) * ks[-1]
            if not st:
                if scheme == RK4:
                    y = x + h / 6 * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
                else:
                    y = x + h * ks[-1]
                st, cur, lam, k = walk(f, y, cur, tol, stats)
            if st:
                state["status"][p] = st
                if st == EXITED:
                    cell = cur
                    state["exit_faces"][p] = exit_face(f.dim, k)
                break
            x, cell, age = y, cur, age + h
        state["positions"][p], state["cells"][p], state["age"][p] = x, cell, age
        state["margin"][p], state["hops"][p] = stats["margin"], stats["hops"]
    return state


def seed(mesh, points, tol=PR.TOL):
    """the state behind nsx_set_tracers: the probes' search; NOT_FOUND: position = seed, cell -1"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, mesh.dim)
    cells, _, _, _ = PR.locate(mesh, pts, tol)
    n = len(pts)
    return {"positions": pts.astype(LD), "cells": cells.copy(), "status": np.where(cells >= 0, ACTIVE, NOT_FOUND).astype(np.int64),
            "exit_faces": np.full(n, -1, dtype=np.int64), "age": np.zeros(n, dtype=LD), "margin": np.full(n, np.inf), "hops": np.zeros(n, dtype=np.int64)}


def run(mesh, dofs, solution, points, dt, n_substeps, scheme, field=FROZEN, previous=None, tol=PR.TOL, calls=1):
    """seed + `calls` advect calls; float64 copies of positions and age beside the long double ones ("positions_ld")"""
    f = Field(mesh, dofs, solution, previous)
    st = seed(mesh, points, tol)
    for _ in range(calls):
        advect(f, st, dt, n_substeps, scheme, field, tol)
    st["positions_ld"] = st["positions"]
    st["positions"] = st["positions"].astype(np.float64)
    st["age"] = st["age"].astype(np.float64)
    return st


# ---- fields with closed-form pathlines
def linear_state(dofs, A, c, b=None):
    """u = A (x - c) + b at the P2 support points, as a solution vector (pressure 0): P2 represents it exactly"""
    dim = dofs.dim
    X = np.asarray(dofs.support_points)[:dofs.n_u:dim]
    u = (X - np.asarray(c)) @ np.asarray(A, dtype=np.float64).T + (0 if b is None else np.asarray(b))
    v = np.zeros(dofs.n_dofs)
    v[:dofs.n_u] = u.ravel()
    return v


def rotation_matrix(dim, omega=1.0):
    A = np.zeros((dim, dim))
    A[0, 1], A[1, 0] = -omega, omega                       # rotation about the z axis
    return A


def linear_closed_form(x0, A, c, h, n, scheme):
    """position after n substeps of size h through u = A (x - c): P^n (x0 - c) + c with P the scheme's polynomial in hA, long double"""
    dim = len(c)
    hA = LD(h) * np.asarray(A, dtype=LD)
    P, term = np.eye(dim, dtype=LD), np.eye(dim, dtype=LD)
    for j in range(1, {EULER: 1, RK2: 2, RK4: 4}[scheme] + 1):
        term = term @ hA / LD(j)
        P = P + term
    Pn = np.eye(dim, dtype=LD)
    for _ in range(n):
        Pn = Pn @ P
    c = np.asarray(c, dtype=LD)
    return (np.asarray(x0, dtype=LD) - c) @ Pn.T + c


def diagonal(mesh):
    V = np.asarray(mesh.vertices)
    return float(np.linalg.norm(V.max(axis=0) - V.min(axis=0)))
