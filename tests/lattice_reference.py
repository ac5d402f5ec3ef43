"""Extended-precision restatement of the lattice sampling (include/nsx.h: nsx_set_lattice / nsx_get_lattice_cells / nsx_eval_lattice /
nsx_get_lattice): the lattice points by the pinned formula origin + i * spacing (one rounded multiply, one rounded add: numpy's float64
arithmetic), located and evaluated through probe_reference.evaluate (np.longdouble, pinned by tests/test_probe_reference.py), the nodal
quantity as the P2 interpolant of given nodal values in np.longdouble.  For lattices too large for the helper's search of every cell for
every point, `raster=True` hands probe_reference.evaluate a search that visits, per cell, only the lattice points near the cell's bounding
box -- the same containment test, the same tie rule; tests/test_lattice_reference.py pins it against the full search.
tests/test_lattice_reference.py pins all of it against closed forms; the GPU tests compare the kernels with it."""
import numpy as np

import diagnostics_reference as R
import nodal_reference as NR
import probe_reference as PR

LD = np.longdouble


def axes(origin, spacing, counts):
    """the coordinates of every axis: origin_d + i * spacing_d in float64, the product rounded before the sum"""
    return [np.float64(origin[d]) + np.arange(int(counts[d]), dtype=np.float64) * np.float64(spacing[d]) for d in range(len(counts))]


def points(origin, spacing, counts):
    """[n_total][dim] lattice points in the order of the linear index i_0 + counts_0 (i_1 + counts_1 i_2): x fastest"""
    ax = axes(origin, spacing, counts)
    grids = np.meshgrid(*ax[::-1], indexing="ij")                                   # shapes counts[::-1]
    return np.stack([g.ravel() for g in grids[::-1]], axis=1)


def span(mesh, counts, overhang=0.0):
    """(origin, spacing) of a lattice of `counts` points over the mesh's bounding box, enlarged by the fraction `overhang` of its extent on
    every side; an axis of one point sits in the middle of the box"""
    V = np.asarray(mesh.vertices, dtype=np.float64)
    lo, hi = V.min(axis=0), V.max(axis=0)
    lo, hi = lo - overhang * (hi - lo), hi + overhang * (hi - lo)
    counts = np.asarray(counts)
    origin = np.where(counts > 1, lo, (lo + hi) / 2)
    spacing = np.where(counts > 1, (hi - lo) / np.maximum(counts - 1, 1), 1.0)
    return origin, spacing


def locate_raster(mesh, origin, spacing, counts, tol=PR.TOL):
    """probe_reference.locate for the lattice, cell by cell over the lattice points within two indices of the cell's bounding box dilated by
    dim tol ext (include/nsx.h derives that bound); returns what locate returns"""
    tol = PR.TOL if tol < 0 else tol
    dim = mesh.dim
    counts = [int(c) for c in counts]
    n = int(np.prod(counts))
    ax = axes(origin, spacing, counts)
    Ji, _ = R.geometry(mesh)
    X = np.asarray(mesh.vertices, dtype=np.float64)[np.asarray(mesh.cells)]          # [nc, nv, dim]
    cells, mult = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    lam = np.zeros((n, dim + 1), dtype=LD)
    stride = np.concatenate([[1], np.cumprod(counts[:-1])]).astype(np.int64)
    for c in range(len(X)):
        vmin, vmax = X[c].min(axis=0), X[c].max(axis=0)
        m = dim * tol * (vmax - vmin)
        lo = np.maximum(np.floor((vmin - m - origin) / spacing).astype(np.int64) - 2, 0)
        hi = np.minimum(np.ceil((vmax + m - origin) / spacing).astype(np.int64) + 2, np.asarray(counts) - 1)
        if (lo > hi).any():
            continue
        idx = np.meshgrid(*[np.arange(lo[d], hi[d] + 1) for d in range(dim)][::-1], indexing="ij")[::-1]
        idx = [g.ravel() for g in idx]
        r = np.stack([ax[d][idx[d]] for d in range(dim)], axis=1).astype(LD) - X[c, 0].astype(LD)     # [m, dim]
        xi = (Ji[c][None, :, :] * r[:, None, :]).sum(axis=2)
        L = np.concatenate([1 - xi.sum(axis=1, keepdims=True), xi], axis=1)
        hit = (L >= -LD(tol)).all(axis=1)
        lin = sum(idx[d][hit] * stride[d] for d in range(dim))
        mult[lin] += 1
        first = cells[lin] < 0                                                       # cells ascend: the first hit is the lowest cell
        cells[lin[first]] = c
        lam[lin[first]] = L[hit][first]
    lam_min = np.where(cells >= 0, lam.min(axis=1).astype(np.float64), -np.inf)
    return cells, lam, mult, lam_min


def evaluate(mesh, dofs, solution, origin, spacing, counts, tol=PR.TOL, raster=False, chunk=65536):
    """probe_reference.evaluate over the lattice points (every array over the linear index); raster: with locate_raster as its search"""
    pts = points(origin, spacing, counts)
    if not raster:
        return PR.evaluate(mesh, dofs, solution, pts, tol)
    found = locate_raster(mesh, origin, spacing, counts, tol)
    keep, parts = PR.locate, []
    try:
        for s in range(0, len(pts), chunk):
            PR.locate = lambda m, p, t=PR.TOL, s=s: tuple(a[s:s + chunk].copy() for a in found)
            parts.append(PR.evaluate(mesh, dofs, solution, pts[s:s + chunk], tol))
    finally:
        PR.locate = keep
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def lambda_in(mesh, pts, cells):
    """[n][dim+1] long double barycentric coordinates of the points in the given cells (0 where cells < 0)"""
    Ji, _ = R.geometry(mesh)
    c = np.where(cells >= 0, cells, 0)
    X0 = np.asarray(mesh.vertices, dtype=LD)[np.asarray(mesh.cells)[c, 0]]
    r = np.asarray(pts, dtype=np.float64).astype(LD) - X0
    xi = (Ji[c] * r[:, None, :]).sum(axis=2)
    lam = np.concatenate([1 - xi.sum(axis=1, keepdims=True), xi], axis=1)
    lam[cells < 0] = 0
    return lam


def interpolate_nodal(mesh, dofs, values, pts, cells):
    """the P2 interpolant sum_a N_a(lambda) V_a of nodal values [n_nodes][n_components] at the points, in the given cells: (value
    [n][n_components] float64, S [n][n_components] = sum_a |N_a| |V_a|); 0 where cells < 0"""
    cells = np.asarray(cells).reshape(-1)
    N, _ = PR.shape_p2(lambda_in(mesh, pts, cells))                                  # [n, np2]
    V = np.asarray(values, dtype=np.float64)[NR.cell_nodes(dofs)[np.where(cells >= 0, cells, 0)]].astype(LD)   # [n, np2, nc]
    val, S = (N[:, :, None] * V).sum(axis=1), (np.abs(N)[:, :, None] * np.abs(V)).sum(axis=1)
    val[cells < 0] = 0
    S[cells < 0] = 0
    return val.astype(np.float64), S.astype(np.float64)


def quadratic_nodal(dofs):
    """a quadratic scalar and a quadratic pair at the P2 nodes [n_nodes][3] -- their P2 interpolants are the polynomials themselves -- and
    the polynomials as a function of points [n][dim]"""
    def q(X):
        X = np.asarray(X)
        x, y = X[:, 0], X[:, 1]
        z = X[:, 2] if X.shape[1] == 3 else 0 * x
        return np.stack([1 + x * x - 3 * x * y + 2 * y + z * z, x - y * y + x * z, 0.5 - y * z + 2 * x], axis=1)
    return q(NR.node_points(dofs)), q


# ---- the lattices of tests/test_gpu_lattice.py, kept here so that tests/test_lattice_reference.py can check on the CPU that they test something
def problem_of(name):
    """arguments of conftest.Problem for the mesh names below"""
    return {"box2": ("box", 2), "box3": ("box", 3), "cube": ("cube", 3, 1), "cyl3": ("cylinder", 3, 1), "cyl2": ("cylinder", 2, 2)}[name]


def owner_cases():
    """name -> (mesh name, counts, overhang or explicit (origin, spacing), tol): the lattices of the owner test, each at most 65536 points"""
    return {
        "box2-255x255": ("box2", (255, 255), 0.0, -1.0),             # boxes of thousands of points: the cooperative path
        "box2-63x5": ("box2", (63, 5), 0.0, -1.0),
        "box2-64x5": ("box2", (64, 5), 0.0, -1.0),
        "box2-65x5": ("box2", (65, 5), 0.0, -1.0),
        "cyl3-5x4x3": ("cyl3", (5, 4, 3), -0.01, -1.0),              # most cells cover no point
        "cyl2-256x64-over": ("cyl2", (256, 64), 0.15, -1.0),         # overhangs the mesh on all sides, covers the hole
        "cyl2-256x64-over-tol0.05": ("cyl2", (256, 64), 0.15, 0.05),  # a dilated acceptance reaches beyond the vertex box
        "cyl2-256x64-over-tol0": ("cyl2", (256, 64), 0.15, 0.0),
        "cube-1x1x1": ("cube", (1, 1, 1), 0.0, -1.0),
        "box3-40x1x30": ("box3", (40, 1, 30), 0.0, -1.0),            # a plane image
        "box2-aligned": ("box2", (7, 7), 0.0, -1.0),                 # on the nodes of the 3 x 3 box mesh: every point is a tie
        "box3-outside": ("box3", (6, 5, 4), ((3.0, -4.0, 2.0), (0.25, 0.25, 0.125)), -1.0),   # wholly outside the mesh
    }


def lattice_of(mesh, case):
    """(origin, spacing, counts, tol) of an owner_cases() entry on its mesh"""
    _, counts, where, tol = case
    if isinstance(where, tuple):
        origin, spacing = np.array(where[0]), np.array(where[1])
    else:
        origin, spacing = span(mesh, counts, where)
    return origin, spacing, np.asarray(counts, dtype=np.int32), tol
