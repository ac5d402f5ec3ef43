"""NumPy restatement of the isosurface extraction (include/nsx.h: nsx_extract_isosurface / nsx_get_isosurface; csrc/nsx_iso.hip): the nodal
scalars in double with the header's formulas, the classification from those doubles, the vertices in np.longdouble from those doubles.  The
case tables are built here from the header's rule (one triangle for 1 or 3 inside vertices, the quad i-k i-l j-l j-k split along its first and
third corner for 2) and oriented by a cross product on the unit simplex -- not copied from host/iso_tables.hpp, which
tests/test_iso_tables.py checks on its own.  tests/test_iso_reference.py pins this file by closed forms; the GPU tests compare the kernels
with it primitive by primitive."""
import numpy as np

import nodal_reference as NR

LD = np.longdouble
VELOCITY, PRESSURE, NODAL, PLANE = range(4)            # NSX_ISO_*
SUB = {2: [(0, 3, 5), (3, 1, 4), (5, 4, 2), (3, 4, 5)],
       3: [(0, 4, 6, 7), (4, 1, 5, 8), (6, 5, 2, 9), (7, 8, 9, 3), (4, 9, 5, 6), (4, 9, 6, 7), (4, 9, 7, 8), (4, 9, 8, 5)]}
LINES = {2: [(0, 1), (1, 2), (2, 0)], 3: [(0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3)]}
UNIT = {2: np.array([[0, 0], [1, 0], [0, 1]], dtype=float), 3: np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=float)}


def source(kind, which=0, component=0, normal=None):
    return {"kind": kind, "which": which, "component": component, "normal": None if normal is None else np.asarray(normal, dtype=np.float64)}


def orientation_ok(dim, prim, inside):
    """on the unit simplex with s = 1 inside, 0 outside, crossings at the mid-points: does the primitive's normal point from inside to
    outside (2D: does the inside lie to the left of p0 -> p1)?"""
    P = UNIT[dim]
    s = np.array([1.0 if v in inside else 0.0 for v in range(dim + 1)])
    g = np.linalg.solve(P[1:] - P[0], s[1:] - s[0])                       # grad s
    p = [0.5 * (P[a] + P[b]) for a, b in prim]
    if dim == 3:
        return float(np.cross(p[1] - p[0], p[2] - p[0]) @ (-g)) > 0
    d = p[1] - p[0]
    return float(np.array([-d[1], d[0]]) @ g) > 0


def case_table(dim):
    """{case: [primitive, ...]}, a primitive = dim crossings (inside vertex, outside vertex) of the sub-simplex, in a cell with det J > 0"""
    table = {}
    for m in range(1 << (dim + 1)):
        ins = [v for v in range(dim + 1) if m >> v & 1]
        out = [v for v in range(dim + 1) if not m >> v & 1]
        if not ins or not out:
            table[m] = []
            continue
        if len(ins) == 1:
            prims = [[(ins[0], o) for o in out]]
        elif len(out) == 1:
            prims = [[(i, out[0]) for i in ins]]
        else:                                                              # tetrahedron, 2 + 2
            (i, j), (k, l) = ins, out
            q = [(i, k), (i, l), (j, l), (j, k)]
            prims = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
        fixed = []
        for p in prims:
            if not orientation_ok(dim, p, ins):
                p = p[:-2] + [p[-1], p[-2]]                                # the last two vertices change places
            assert orientation_ok(dim, p, ins)
            fixed.append(p)
        table[m] = fixed
    return table


TABLE = {2: case_table(2), 3: case_table(3)}


def cell_det(dofs):
    """det J of every cell, in double, by the expression of the library's mesh set-up"""
    X = np.asarray(dofs.cell_coords, dtype=np.float64)
    J = np.swapaxes(X[:, 1:, :] - X[:, :1, :], 1, 2)                       # J[d][k] = X[k + 1][d] - X[0][d]
    if dofs.dim == 2:
        return J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    return (J[:, 0, 0] * (J[:, 1, 1] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 1]) - J[:, 0, 1] * (J[:, 1, 0] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 0]) +
            J[:, 0, 2] * (J[:, 1, 0] * J[:, 2, 1] - J[:, 1, 1] * J[:, 2, 0]))


def nodal_scalar(dofs, solution, src, nodal=None):
    """[n_nodes] float64: the scalar of `src` at every P2 node (caller's numbering), every operation in double and in the header's order.
    nodal: {NR.NAMES[which]: array [n_nodes][...]} for NSX_ISO_NODAL (the values the device holds, as nsx_get_nodal_field returns them)"""
    dim = dofs.dim
    n_nodes = dofs.n_u // dim
    u = np.asarray(solution, dtype=np.float64)
    kind = src["kind"]
    if kind == VELOCITY:
        U = u[:dofs.n_u].reshape(n_nodes, dim)
        if src["component"] >= 0:
            return U[:, src["component"]].copy()
        ss = np.zeros(n_nodes)
        for i in range(dim):
            ss = ss + U[:, i] * U[:, i]
        return np.sqrt(ss)
    if kind == PRESSURE:
        cd, cn = np.asarray(dofs.cell_dofs), NR.cell_nodes(dofs)
        P = u[cd[:, [(dim + 1) * v + dim for v in range(dim + 1)]]]         # [nc][dim+1] the P1 values at the vertices
        s = np.full(n_nodes, np.nan)
        for v in range(dim + 1):
            s[cn[:, v]] = P[:, v]
        for e, (i, j) in enumerate(LINES[dim]):
            s[cn[:, dim + 1 + e]] = 0.5 * (P[:, i] + P[:, j])
        return s
    if kind == NODAL:
        a = np.asarray(nodal[NR.NAMES[src["which"]]], dtype=np.float64).reshape(n_nodes, -1)
        return a[:, src["component"]].copy()
    if kind == PLANE:
        X = NR.node_points(dofs)
        s = np.zeros(n_nodes)
        for d in range(dim):
            s = s + src["normal"][d] * X[:, d]
        return s
    raise ValueError(kind)


def extract(dofs, solution, field, iso, colour=None, nodal=None, counted=None):
    """The primitives of { field = iso } in the order of nsx_get_isosurface.  dict:
    points [n][dim][dim] float64 (rounded from points_ld), colour [n][dim] or None, cells [n] int32, sub [n], s [n_nodes] the field's
    nodal scalars, t [n][dim] (float64), node_a / node_b [n][dim] the inside / outside node of every vertex,
    bound_x [n][dim][dim] = |x_a| + |x_b| componentwise, bound_c [n][dim] = |c_a| + |c_b|
    counted: bool [n_cells], the cells to extract from (default: all)"""
    dim = dofs.dim
    cn = NR.cell_nodes(dofs)
    nc = len(cn)
    X = NR.node_points(dofs)
    s = nodal_scalar(dofs, solution, field, nodal)
    c = nodal_scalar(dofs, solution, colour, nodal) if colour is not None else None
    flip = cell_det(dofs) < 0
    counted = np.ones(nc, dtype=bool) if counted is None else np.asarray(counted, dtype=bool)
    iso = np.float64(iso)
    keys, NA, NB = [], [], []
    for sub, loc in enumerate(SUB[dim]):
        nodes = cn[:, loc]                                                  # [nc][dim+1]
        S = s[nodes]
        fin = np.isfinite(S).all(axis=1)
        with np.errstate(invalid="ignore"):
            case = ((S >= iso) << np.arange(dim + 1)).sum(axis=1)
        for m, prims in TABLE[dim].items():
            if not prims:
                continue
            sel = np.nonzero(fin & counted & (case == m))[0]
            if len(sel) == 0:
                continue
            for t, prim in enumerate(prims):
                na = np.stack([nodes[sel, a] for a, _ in prim], axis=1)    # [k][dim]
                nb = np.stack([nodes[sel, b] for _, b in prim], axis=1)
                f = flip[sel]
                order = np.arange(dim)[None, :].repeat(len(sel), axis=0)
                order[f, -2], order[f, -1] = dim - 1, dim - 2
                na, nb = np.take_along_axis(na, order, axis=1), np.take_along_axis(nb, order, axis=1)
                keys.append(np.stack([sel, np.full(len(sel), sub), np.full(len(sel), t)], axis=1))
                NA.append(na)
                NB.append(nb)
    if keys:
        keys, NA, NB = np.concatenate(keys), np.concatenate(NA), np.concatenate(NB)
        o = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        keys, NA, NB = keys[o], NA[o], NB[o]
    else:
        keys, NA, NB = np.zeros((0, 3), dtype=np.int64), np.zeros((0, dim), dtype=np.int64), np.zeros((0, dim), dtype=np.int64)
    sa, sb = s[NA].astype(LD), s[NB].astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (sa - LD(iso)) / (sa - sb)                                      # [n][dim]
    xa, xb = X[NA].astype(LD), X[NB].astype(LD)                            # [n][dim][dim]
    pts = xa + t[:, :, None] * (xb - xa)
    out = {"points_ld": pts, "points": pts.astype(np.float64), "cells": keys[:, 0].astype(np.int32), "sub": keys[:, 1].astype(np.int32), "s": s, "t": t.astype(np.float64),
           "node_a": NA, "node_b": NB, "bound_x": np.abs(X[NA]) + np.abs(X[NB]), "colour": None, "bound_c": None}
    if c is not None:
        ca, cb = c[NA].astype(LD), c[NB].astype(LD)
        col = ca + t * (cb - ca)
        out.update(colour_ld=col, colour=col.astype(np.float64), bound_c=np.abs(c[NA]) + np.abs(c[NB]), c=c)
    return out


# ------------------------------------------------------------------ measures and topology of a soup
def measure(points):
    """[n] length of every segment / area of every triangle (the float type of `points`)"""
    p = np.asarray(points)
    if p.shape[1] == 2:
        d = p[:, 1] - p[:, 0]
        return np.sqrt((d * d).sum(axis=1))
    n = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return np.sqrt((n * n).sum(axis=1)) / 2


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def normals(points):
    """[n][3] (p1 - p0) x (p2 - p0) of every triangle; 2D: [n][2] the left normal of p0 -> p1"""
    p = np.asarray(points, dtype=np.float64)
    if p.shape[1] == 2:
        d = p[:, 1] - p[:, 0]
        return np.stack([-d[:, 1], d[:, 0]], axis=1)
    return _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def edge_census(points):
    """The directed edges of a triangle soup with their vertices compared AS BYTES (float64).  Returns (n_vertices, undirected, directed):
    undirected {frozenset of two vertex keys: occurrences}, directed {(key, key): occurrences}; primitives of zero extent (two equal
    vertices) are left out."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    p = p + 0.0                                                              # -0.0 and 0.0 are one point
    keys = [[p[i, v].tobytes() for v in range(3)] for i in range(len(p))]
    und, dire, verts = {}, {}, set()
    for k in keys:
        if len(set(k)) < 3:
            continue
        verts.update(k)
        for a, b in ((k[0], k[1]), (k[1], k[2]), (k[2], k[0])):
            dire[(a, b)] = dire.get((a, b), 0) + 1
            e = frozenset((a, b))
            und[e] = und.get(e, 0) + 1
    return len(verts), und, dire


def is_closed_oriented(points):
    """every undirected edge twice, once in each direction; returns (closed, V - E + F)"""
    nv, und, dire = edge_census(points)
    closed = all(v == 2 for v in und.values()) and all(v == 1 for v in dire.values())
    p = np.ascontiguousarray(points, dtype=np.float64) + 0.0
    f = sum(1 for i in range(len(p)) if len({p[i, v].tobytes() for v in range(3)}) == 3)
    return closed, nv - len(und) + f


def sub_volumes(dofs):
    """[n_cells][n_sub] signed volume of every sub-simplex over the signed volume of its cell"""
    dim = dofs.dim
    cn = NR.cell_nodes(dofs)
    X = NR.node_points(dofs).astype(LD)

    def vol(P):                                                              # [nc][dim+1][dim]
        J = P[:, 1:, :] - P[:, :1, :]
        if dim == 2:
            return J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        return (J[:, 0] * _cross(J[:, 1], J[:, 2])).sum(axis=1)
    whole = vol(X[cn[:, :dim + 1]])
    return np.stack([vol(X[cn[:, loc]]) / whole for loc in SUB[dim]], axis=1)
