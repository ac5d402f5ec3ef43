"""Extended-precision restatement of the flow diagnostics (include/nsx.h, nsx_compute_diagnostics / nsx_get_cell_diagnostic), written
like problem.py: velocity_error: J, J^-1 and |det J| from the vertices, everything per cell accumulated in np.longdouble, the totals
with math.fsum.  tests/test_diagnostics_reference.py pins it against closed forms; the GPU tests compare the kernels with it."""
import math

import numpy as np

KEYS = ("kinetic_energy", "div2", "grad_l2_sq", "enstrophy", "change2", "volume", "cfl_max", "speed_max")  # order of NSX_DIAG_*
ENERGY, DIV2, GRAD2, ENSTROPHY, CHANGE2, VOLUME, CFL, SPEED = range(8)
LD = np.longdouble


def geometry(mesh):
    """J^-1 [nc][k][d] and |det J| [nc] of the affine maps, by cofactors in long double"""
    dim = mesh.dim
    X = np.asarray(mesh.vertices, dtype=LD)[np.asarray(mesh.cells)]      # [nc, nv, dim]
    J = np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))                     # J[d][k] = x_{k+1,d} - x_{0,d}
    nc = J.shape[0]
    Ji = np.zeros((nc, dim, dim), dtype=LD)
    if dim == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        Ji[:, 0, 0], Ji[:, 0, 1], Ji[:, 1, 0], Ji[:, 1, 1] = J[:, 1, 1], -J[:, 0, 1], -J[:, 1, 0], J[:, 0, 0]
    else:
        def cof(i, j):  # cofactor of J[i][j]
            r = [a for a in range(3) if a != i]
            c = [a for a in range(3) if a != j]
            return (-1) ** (i + j) * (J[:, r[0], c[0]] * J[:, r[1], c[1]] - J[:, r[0], c[1]] * J[:, r[1], c[0]])
        det = sum(J[:, 0, j] * cof(0, j) for j in range(3))
        for i in range(3):
            for j in range(3):
                Ji[:, j, i] = cof(i, j)                                  # inverse = adjugate / det = cofactor^T / det
    Ji /= det[:, None, None]
    return Ji, np.abs(det)


def cell_velocities(dofs, vector):
    """[nc][n_p2][dim] nodal velocities of every cell (FESystem local order: vertices, then lines)"""
    dim = dofs.dim
    nv = dim + 1
    np2 = 6 if dim == 2 else 10
    base = [(dim + 1) * a if a < nv else nv * (dim + 1) + dim * (a - nv) for a in range(np2)]
    cd = np.asarray(dofs.cell_dofs)
    v = np.asarray(vector, dtype=np.float64)
    return np.stack([v[cd[:, [b + c for b in base]]] for c in range(dim)], axis=2).astype(LD)


def flow_diagnostics(mesh, dofs, tables, solution, previous, deltat):
    """{"cells": float64 [8][n_cells] in the order of NSX_DIAG_*, "totals": the fields of nsx_flow_diag}"""
    dim = mesh.dim
    Ji, adet = geometry(mesh)
    U = cell_velocities(dofs, solution)
    D = U - cell_velocities(dofs, previous)
    nc = U.shape[0]
    N, dN, w = (np.asarray(t, dtype=LD) for t in (tables.N2, tables.dN2, tables.weights))
    acc = np.zeros((8, nc), dtype=LD)
    for q in range(tables.n_q):
        jxw = adet * w[q]
        u = sum(N[q, a] * U[:, a, :] for a in range(tables.n_p2))                                   # [nc, dim]
        d = sum(N[q, a] * D[:, a, :] for a in range(tables.n_p2))
        # G[c][i][j] = sum_a U_a,i (J^-T grad_hat N_a)_j = d_j u_i
        G = sum(U[:, a, :, None] * sum(dN[q, a, k] * Ji[:, k, None, :] for k in range(dim)) for a in range(tables.n_p2))
        ut = np.stack([sum(Ji[:, k, i] * u[:, i] for i in range(dim)) for k in range(dim)], axis=1)  # u_q . grad lambda_k, k = 1..dim
        lam = np.concatenate([-ut.sum(axis=1, keepdims=True), ut], axis=1)
        uu = (u * u).sum(axis=1)
        div = sum(G[:, i, i] for i in range(dim))
        if dim == 2:
            curl2 = (G[:, 1, 0] - G[:, 0, 1]) ** 2
        else:
            curl2 = (G[:, 2, 1] - G[:, 1, 2]) ** 2 + (G[:, 0, 2] - G[:, 2, 0]) ** 2 + (G[:, 1, 0] - G[:, 0, 1]) ** 2
        acc[ENERGY] += uu * jxw / 2
        acc[DIV2] += div * div * jxw
        acc[GRAD2] += (G * G).sum(axis=(1, 2)) * jxw
        acc[ENSTROPHY] += curl2 * jxw / 2
        acc[CHANGE2] += (d * d).sum(axis=1) * jxw
        acc[VOLUME] += jxw
        acc[CFL] = np.maximum(acc[CFL], np.abs(lam).max(axis=1))
        acc[SPEED] = np.maximum(acc[SPEED], uu)
    acc[CFL] *= LD(deltat)
    acc[SPEED] = np.sqrt(acc[SPEED])
    cells = acc.astype(np.float64)
    s = [math.fsum(cells[p]) for p in range(6)]
    totals = {"kinetic_energy": s[ENERGY], "div_l2": math.sqrt(s[DIV2]), "grad_l2_sq": s[GRAD2], "enstrophy": s[ENSTROPHY],
              "change_l2": math.sqrt(s[CHANGE2]), "volume": s[VOLUME], "cfl_max": float(cells[CFL].max()),
              "speed_max": float(cells[SPEED].max()), "n_cells": nc}
    return {"cells": cells, "totals": totals}


# ---- the quadratic field of the known-answer tests and its closed-form integrals over a box [0, hi]
def quadratic_field(X):
    """u and grad u (G[i][j] = d_j u_i) at the points X [n][dim]: u = (x^2 - yz, -2xy + z^2, y + xz) in 3D; in 2D
    u = (x^2 - y/2, -xy + y^2) (the 3D field cut down to z = 0 is divergence-free, which would leave nothing to compare div with)."""
    X = np.asarray(X)
    n, dim = X.shape
    G = np.zeros((n, dim, dim), dtype=X.dtype)
    x, y = X[:, 0], X[:, 1]
    if dim == 2:
        u = np.stack([x * x - y / 2, -x * y + y * y], axis=1)
        G[:, 0, 0], G[:, 0, 1] = 2 * x, -0.5
        G[:, 1, 0], G[:, 1, 1] = -y, -x + 2 * y
    else:
        z = X[:, 2]
        u = np.stack([x * x - y * z, -2 * x * y + z * z, y + x * z], axis=1)
        G[:, 0, 0], G[:, 0, 1], G[:, 0, 2] = 2 * x, -z, -y
        G[:, 1, 0], G[:, 1, 1], G[:, 1, 2] = -2 * y, -2 * x, 2 * z
        G[:, 2, 0], G[:, 2, 1], G[:, 2, 2] = z, 1, x
    return u, G


def interpolate_quadratic(dofs):
    """the field at the P2 support points, as a solution vector (pressure 0): its P2 interpolant is the field itself"""
    dim = dofs.dim
    X = np.asarray(dofs.support_points)
    v = np.zeros(dofs.n_dofs)
    u, _ = quadratic_field(X[:dofs.n_u])
    v[:dofs.n_u] = u[np.arange(dofs.n_u), np.arange(dofs.n_u) % dim]
    return v


def quadratic_closed_forms(hi, lo=None, n_gauss=4):
    """kinetic energy, int (div u)^2, int |grad u|^2, enstrophy of the quadratic field over the box [lo, hi] (lo = 0 by default): tensor
    Gauss-Legendre with n_gauss points per direction (exact to degree 2 n_gauss - 1 >= 4 = the degree of |u|^2), summed in long double"""
    dim = len(hi)
    lo = [0.0] * dim if lo is None else lo
    t, w = np.polynomial.legendre.leggauss(n_gauss)
    axes = [(LD(a) + (LD(b) - LD(a)) * (LD(1) + t.astype(LD)) / 2, (LD(b) - LD(a)) * w.astype(LD) / 2) for a, b in zip(lo, hi)]
    P = np.stack(np.meshgrid(*[a[0] for a in axes], indexing="ij"), axis=-1).reshape(-1, dim)
    W = np.ones(1, dtype=LD)
    for a in axes:
        W = np.multiply.outer(W, a[1])
    W = W.reshape(-1)
    u, G = quadratic_field(P)
    div = sum(G[:, i, i] for i in range(dim))
    if dim == 2:
        curl2 = (G[:, 1, 0] - G[:, 0, 1]) ** 2
    else:
        curl2 = (G[:, 2, 1] - G[:, 1, 2]) ** 2 + (G[:, 0, 2] - G[:, 2, 0]) ** 2 + (G[:, 1, 0] - G[:, 0, 1]) ** 2
    return {"kinetic_energy": float((W * (u * u).sum(axis=1)).sum() / 2), "div2": float((W * div * div).sum()),
            "grad_l2_sq": float((W * (G * G).sum(axis=(1, 2))).sum()), "enstrophy": float((W * curl2).sum() / 2),
            "volume": float(np.prod(np.asarray(hi, dtype=LD) - np.asarray(lo, dtype=LD)))}


def smooth_field(dofs):
    """a divergence-carrying velocity that depends on the position of a node only (not on its number): the same field on every
    numbering and partition of one mesh; pressure 0"""
    dim = dofs.dim
    X = np.asarray(dofs.support_points)
    v = np.zeros(dofs.n_dofs)
    for c in range(dim):
        Xc = X[c:dofs.n_u:dim]
        v[c:dofs.n_u:dim] = (c + 1) * Xc[:, 1] * (0.41 - Xc[:, 1]) + 0.3 * np.sin(3 * Xc[:, 0] + c) + 0.05 * np.cos(40 * Xc[:, 0] * Xc[:, 1] + 7 * c)
    return v
