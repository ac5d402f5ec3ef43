"""Extended-precision restatement of the nodal fields (include/nsx.h: nsx_compute_nodal_fields / nsx_get_nodal_field), in the manner of
tests/probe_reference.py: the patches from dofs.cell_dofs, grad u_h per (cell, local node) with the barycentric P2 gradients
(probe_reference.shape_p2) and J^-1, |det J| by cofactors (diagnostics_reference.geometry), everything in np.longdouble, the volume-weighted
sums folded in ascending cell order.  tests/test_nodal_reference.py pins it against closed forms; the GPU tests compare the kernel with it."""
import numpy as np

import diagnostics_reference as R
import probe_reference as PR

LD = np.longdouble
NAMES = ("gradient", "vorticity", "q", "strain", "divergence")   # order of NSX_FIELD_*


def cell_nodes(dofs):
    """[nc][n_p2] P2 node of every local node (FESystem local order: vertices, then lines); node i carries the velocity dofs dim i ..."""
    dim = dofs.dim
    nv = dim + 1
    np2 = 6 if dim == 2 else 10
    base = [(dim + 1) * a if a < nv else nv * (dim + 1) + dim * (a - nv) for a in range(np2)]
    return np.asarray(dofs.cell_dofs)[:, base] // dim


def node_lambda(dim):
    """[n_p2][dim+1] barycentric position of every local node: e_k for vertex k, (e_i + e_j) / 2 for the line {i, j}"""
    nv = dim + 1
    lam = np.zeros((nv + len(PR.LINES[dim]), nv), dtype=LD)
    for a in range(nv):
        lam[a, a] = 1
    for e, (i, j) in enumerate(PR.LINES[dim]):
        lam[nv + e, i] = lam[nv + e, j] = LD(1) / 2
    return lam


def patch_holds(dofs, dof):
    """bool [n_nodes]: the nodes whose patch holds velocity dof `dof` (some cell that holds the node holds the dof's node as well)"""
    cn = cell_nodes(dofs)
    out = np.zeros(dofs.n_u // dofs.dim, dtype=bool)
    out[np.unique(cn[(cn == dof // dofs.dim).any(axis=1)])] = True
    return out


def derive(G):
    """the four derived fields of G [n][dim][dim] (any float type): vorticity [n][3 | 1], q [n], strain [n], divergence [n]"""
    dim = G.shape[1]
    S, W = (G + np.swapaxes(G, 1, 2)) / 2, (G - np.swapaxes(G, 1, 2)) / 2
    if dim == 3:
        vort = np.stack([G[:, 2, 1] - G[:, 1, 2], G[:, 0, 2] - G[:, 2, 0], G[:, 1, 0] - G[:, 0, 1]], axis=1)
    else:
        vort = (G[:, 1, 0] - G[:, 0, 1])[:, None]
    return {"vorticity": vort, "q": ((W * W).sum(axis=(1, 2)) - (S * S).sum(axis=(1, 2))) / 2, "strain": np.sqrt(2 * (S * S).sum(axis=(1, 2))),
            "divergence": sum(G[:, i, i] for i in range(dim))}


def propagate(G, strain, SG, prefix):
    """the absolute-term sums SG [n][dim][dim] of the gradient carried to first order through the formulas of the derived fields"""
    dim = G.shape[1]
    if dim == 3:
        S_vort = np.stack([SG[:, 2, 1] + SG[:, 1, 2], SG[:, 0, 2] + SG[:, 2, 0], SG[:, 1, 0] + SG[:, 0, 1]], axis=1)
    else:
        S_vort = (SG[:, 1, 0] + SG[:, 0, 1])[:, None]
    Ssym = np.abs(G + np.swapaxes(G, 1, 2)) / 2
    first = 2 * (Ssym * SG).sum(axis=(1, 2)) / np.where(strain > 0, strain, 1)
    out = {"gradient": SG, "vorticity": S_vort, "q": (np.abs(G) * np.swapaxes(SG, 1, 2)).sum(axis=(1, 2)),
           "strain": np.where(strain > 0, first, np.sqrt(LD(2)) * SG.sum(axis=(1, 2))), "divergence": sum(SG[:, i, i] for i in range(dim))}
    return {prefix + k: v.astype(np.float64) for k, v in out.items()}


def nodal_fields(mesh, dofs, solution):
    """dict over the P2 nodes (caller's numbering):
    gradient [n][dim][dim] (Gbar_ij = d_j u_i), vorticity [n][3 | 1], q [n], strain [n], divergence [n]      float64
    the same keys with the suffix "_ld": np.longdouble, before rounding
    patch_size [n]
    S_gradient [n][dim][dim]    the absolute-term sum S_G,ij = sum_c |c| sum_a |U_a,i| |d_j N_a| / sum_c |c|
    S_vorticity, S_q, S_strain, S_divergence    S_G propagated to first order through the formula of the field: linear fields the sum of the
        S_G entries involved; q: sum_ij |Gbar_ij| S_G,ji; strain: (2 / strain) sum_ij |S_ij| S_G,ij, and sqrt(2) sum_ij S_G,ij where the
        strain is 0
    X_gradient, X_vorticity, ...    the same with the absolute terms of the library's ORDER of evaluation (reference derivatives first, J^-1
        last, as nsx_eval_probes): X_G,ij = sum_c |c| sum_q (sum_a |U_a,i| |d N_a / d xi_q|) |J^-1_qj| / sum_c |c| >= S_G,ij.  The two differ
        where the physical derivative of a shape function vanishes by cancellation between the rows of J^-1 (a face parallel to an axis):
        such a node adds nothing to S_G,ij but its rounding errors are those of the terms of X_G,ij"""
    dim = mesh.dim
    n_nodes = dofs.n_u // dim
    cn = cell_nodes(dofs)                                                            # [nc, np2]
    nc, np2 = cn.shape
    Ji, adet = R.geometry(mesh)                                                      # [nc, k, d], [nc]
    U = R.cell_velocities(dofs, solution)                                            # [nc, np2, dim]
    _, dN = PR.shape_p2(node_lambda(dim))                                            # [np2 (where), np2 (which N), k]
    gN = (dN[None, :, :, :, None] * Ji[:, None, None, :, :]).sum(axis=3)             # [nc, where, a, j] physical gradient of N_a
    Gc = (U[:, None, :, :, None] * gN[:, :, :, None, :]).sum(axis=2)                 # [nc, where, i, j]
    Sc = (np.abs(U)[:, None, :, :, None] * np.abs(gN)[:, :, :, None, :]).sum(axis=2)
    aH = (np.abs(U)[:, None, :, :, None] * np.abs(dN)[None, :, :, None, :]).sum(axis=2)   # [nc, where, i, q] sum_a |U_a,i| |d N_a / d xi_q|
    Xc = (aH[:, :, :, :, None] * np.abs(Ji)[:, None, None, :, :]).sum(axis=3)            # [nc, where, i, j]
    vol = adet * (LD(1) / (2 if dim == 2 else 6))
    num, sab, xab = (np.zeros((n_nodes, dim, dim), dtype=LD) for _ in range(3))
    den = np.zeros(n_nodes, dtype=LD)
    size = np.zeros(n_nodes, dtype=np.int64)
    for c in range(nc):                                                              # ascending cell order, left to right
        n = cn[c]                                                                    # (the nodes of one cell are distinct)
        num[n] += vol[c] * Gc[c]
        sab[n] += vol[c] * Sc[c]
        xab[n] += vol[c] * Xc[c]
        den[n] += vol[c]
        size[n] += 1
    held = size > 0
    safe = np.where(held, den, 1)
    G = np.where(held[:, None, None], num / safe[:, None, None], 0)
    out = {"gradient_ld": G, "patch_size": size}
    out.update({k + "_ld": v for k, v in derive(G).items()})
    for prefix, acc in (("S_", sab), ("X_", xab)):
        out.update(propagate(G, out["strain_ld"], np.where(held[:, None, None], acc / safe[:, None, None], 0), prefix))
    for k in NAMES:
        out[k] = out[k + "_ld"].astype(np.float64)
    return out


def node_points(dofs):
    """[n_nodes][dim] support point of every P2 node"""
    return np.asarray(dofs.support_points)[:dofs.n_u:dofs.dim].copy()


def interpolate(dofs, field):
    """field(X [n][dim]) -> u [n][dim] at the P2 support points, as a solution vector (pressure 0)"""
    v = np.zeros(dofs.n_dofs)
    v[:dofs.n_u] = np.asarray(field(node_points(dofs)), dtype=np.float64).reshape(-1)
    return v
