"""Extended-precision restatement of the surface loads (include/nsx.h, section "surface loads": nsx_set_surface / nsx_compute_surface /
nsx_get_surface_field), in the manner of tests/nodal_reference.py: geometry by cofactors from the vertices, the barycentric P2 evaluation of
tests/probe_reference.py at the nodes of every face, traction, shear and y+, the area-weighted recovery at the surface nodes folded in
ascending face order, and the totals per group by the P2 nodal rule of the face.  Everything once in np.longdouble and once in plain float64
in the library's order of evaluation (reference derivatives first, J^-1 last; the totals folded in the library's tree).
tests/test_surface_reference.py pins it against closed forms; the GPU tests compare the kernels with it.

Absolute-term sums.  Beside every value the helper returns X: the same evaluation with every input replaced by its absolute value and every
difference by a sum, from the vertex differences on (the cofactors and the determinant of J included; lengths and denominators are the true
ones) -- the sum of the absolute terms in the library's order of evaluation, the scale its rounding errors have (tests/test_gpu_nodal_fields.py,
docstring of test_the_call_changes_no_state_..., says why X and not the sum S of the physical terms).  Fields are compared under the project's
standing 1e-12 X.  Non-linear fields to first order: X_|s| = sum_i |s_i| X_s,i / |s| (sqrt(sum X_s^2) where s = 0);
X_y+ = (X_|s| / (2 sqrt|s|) d + sqrt|s| X_d) / nu.  Where |s| = 0 < X_|s| (the quadratic state on a box has such nodes) the square root has
no first order: a computed |s| within 1e-12 X_|s| of 0 gives a y+ within sqrt(1e-12 X_|s|) X_d / nu of 0, so there
X_y+ = sqrt(X_|s| / TOL) X_d / nu with TOL = 1e-12 -- the standing tolerance on |s| carried through the root; no entry is exempted.

Bound of the totals.  For a total T = fold_f sum_j w_j term_j the helper returns A = sum_f sum_j X(w_j term_j).  In double arithmetic, unit
roundoff u = 2^-53, a value that is reached from the vertex coordinates through k rounded operations, each on terms whose absolute values X
accounts for, is off by at most (k + O(k^2 u)) u X.  The longest chain is the torque in 3D with the symmetric stress; counted per operand:
  J entry 1; cofactor 2 (its J entries) + 3 = 5; det 1 + 5 + 1 + 2 = 9; J^-1 entry 5 + 9 + 1 = 15;
  H = sum_a U_a dN_a: 10;  G = H J^-1: 10 + 15 + 1 + 2 = 28;  tau = nu (G + G^T): 30;
  grad lambda_0 = -(row + row + row): 17;  |grad lambda|: 20;  n: 17 + 20 + 1 = 38;  tau n: 30 + 38 + 1 + 2 = 71;  t = p n - tau n: 72;
  |f| = |det J| |grad lambda| / 2: 9 + 20 + 2 = 31;  w = |f| / 3: 32;  r = x - centre: 2;  r x t: 72 + 2 + 1 + 1 = 76;  w (r x t): 76 + 32 + 1 = 109;
  the three nodes of the face: + 2 = 111
so every chain has fewer than C1 = 128 rounded operations, and the fold of a group adds one addition per level of its tree, 6 per launch
level of 64 entries: |T_double - T| <= (C1 + depth) u A for any evaluation in double that follows the library's order, fused or not (a fused
multiply-add rounds once where the count above has two).  The float64 run below and the device are two such evaluations; a long double run
(u = 2^-64) stands for T.  total_bound() returns the right-hand side."""
import numpy as np

import diagnostics_reference as R
import nodal_reference as NR
import probe_reference as PR

LD = np.longdouble
FIELDS = ("pressure", "traction", "shear", "shear_magnitude", "normal", "yplus")      # order of NSX_SURFACE_*
NODE_FIELDS = FIELDS[:5]
TOTALS = ("area", "force_pressure", "force_viscous", "torque", "flux", "pressure_integral")
SYMMETRIC, GRADIENT = 0, 1
FACE_VERTICES = {2: [(0, 1), (1, 2), (2, 0)], 3: [(0, 1, 2), (1, 0, 3), (0, 2, 3), (2, 1, 3)]}   # deal.II local face -> local vertices
FOLD = 64                                                                             # entries per block of the library's fold
C1 = 128
TOL = 1e-12                                                                           # the standing tolerance of the fields (X_y+ at |s| = 0)


def opposite_vertex(dim, lf):
    """the local vertex the deal.II local face lf lies opposite of"""
    return 3 - lf if dim == 3 else (lf + 2) % 3


def face_local_nodes(dim):
    """[dim+1][3 | 6] local P2 node of every face node: the face's vertices, then the lines v0 v1, v1 v2, v2 v0 (2D: the one line)"""
    nv = dim + 1

    def line(i, j):
        return nv + next(e for e, (a, b) in enumerate(PR.LINES[dim]) if {a, b} == {i, j})
    out = []
    for fv in FACE_VERTICES[dim]:
        edges = [(fv[0], fv[1])] if dim == 2 else [(fv[0], fv[1]), (fv[1], fv[2]), (fv[2], fv[0])]
        out.append(list(fv) + [line(i, j) for i, j in edges])
    return np.array(out)


def layout(dofs, cells, lfs, groups):
    """the surface-node table: nodes [n_s] (P2 node), node_groups [n_s], face_nodes [n_f][npf]; surface nodes by ascending (group, node)"""
    cn = NR.cell_nodes(dofs)
    loc = face_local_nodes(dofs.dim)[np.asarray(lfs)]                                 # [nf, npf]
    node = cn[np.asarray(cells)[:, None], loc]
    key = np.asarray(groups, dtype=np.int64)[:, None] * (int(cn.max()) + 1) + node
    uniq, inv = np.unique(key.ravel(), return_inverse=True)
    return {"nodes": (uniq % (int(cn.max()) + 1)).astype(np.int64), "node_groups": (uniq // (int(cn.max()) + 1)).astype(np.int64),
            "face_nodes": inv.reshape(key.shape), "local_nodes": loc}


def _cofactors(J, ab):
    """cofactor matrix C [nf][i][j] and the determinant by the first row (ab: sums of absolute terms)"""
    dim = J.shape[1]
    sub = (lambda a, b: a + b) if ab else (lambda a, b: a - b)
    C = np.zeros_like(J)
    if dim == 2:
        C[:, 0, 0], C[:, 0, 1], C[:, 1, 0], C[:, 1, 1] = J[:, 1, 1], J[:, 1, 0] if ab else -J[:, 1, 0], J[:, 0, 1] if ab else -J[:, 0, 1], J[:, 0, 0]
        det = sub(J[:, 0, 0] * J[:, 1, 1], J[:, 0, 1] * J[:, 1, 0])
        return C, det
    for i in range(3):
        for j in range(3):
            r, c = [a for a in range(3) if a != i], [a for a in range(3) if a != j]
            m = sub(J[:, r[0], c[0]] * J[:, r[1], c[1]], J[:, r[0], c[1]] * J[:, r[1], c[0]])
            C[:, i, j] = m if ab or (i + j) % 2 == 0 else -m
    det = sum(J[:, 0, j] * C[:, 0, j] for j in range(3))
    return C, det


def _evaluate(dim, Xv, U, P, lfs, nu, form, centre, T, true=None):
    """the face-node values and the per-face contributions to the totals in the float type T.  true = None: the values; true = the result of
    the value run: the absolute-term sums (inputs by absolute value, differences as sums, lengths and denominators from `true`)."""
    ab = true is not None
    nv, nf = dim + 1, len(lfs)
    sub = (lambda a, b: a + b) if ab else (lambda a, b: a - b)
    Xv, U, P = Xv.astype(T), U.astype(T), P.astype(T)
    J = np.transpose(Xv[:, 1:] - Xv[:, :1], (0, 2, 1))                                # J[d][k] = x_{k+1,d} - x_{0,d}: one rounding each
    if ab:
        J, U, P = np.abs(J), np.abs(U), np.abs(P)
    C, det = _cofactors(J, ab)
    if ab:                                                                            # the error of cof / det relative to the true |det|
        Ji = np.transpose(C, (0, 2, 1)) * (det / true["det"] ** 2)[:, None, None]
        adet = det
    else:
        Ji = np.transpose(C, (0, 2, 1)) / det[:, None, None]                          # inverse = cofactor^T / det; Ji[k][d]
        adet = np.abs(det)
    k = np.array([opposite_vertex(dim, int(l)) for l in lfs])
    rows = Ji[:, 0, :].copy()
    for r in range(1, dim):
        rows = rows + Ji[:, r, :]
    gl = np.where((k == 0)[:, None], rows if ab else -rows, Ji[np.arange(nf), np.maximum(k, 1) - 1, :])
    length = np.sqrt((gl * gl).sum(axis=1))
    if ab:
        n, d = gl * (length / true["len"] ** 2)[:, None], length / true["len"] ** 2
    else:
        n, d = -gl / length[:, None], 1 / length
    area = adet * length * T(1 if dim == 2 else 0.5)
    loc = face_local_nodes(dim)[np.asarray(lfs)]                                      # [nf, npf]
    npf = loc.shape[1]
    lam = NR.node_lambda(dim)[loc]                                                    # [nf, npf, nv], exact
    N, dN = PR.shape_p2(lam.reshape(-1, nv))
    N, dN = N.reshape(nf, npf, -1).astype(T), dN.reshape(nf, npf, -1, dim).astype(T)  # small integers and halves: exact in any type
    lamT = lam.astype(T)
    if ab:
        N, dN = np.abs(N), np.abs(dN)
    p = (lamT * P[:, None, :]).sum(axis=2)                                            # [nf, npf]
    u = (N[:, :, :, None] * U[:, None, :, :]).sum(axis=2)                             # [nf, npf, i]
    H = (U[:, None, :, :, None] * dN[:, :, :, None, :]).sum(axis=2)                   # [nf, npf, i, k]
    G = (H[:, :, :, :, None] * Ji[:, None, None, :, :]).sum(axis=3)                   # [nf, npf, i, c]
    nuT = T(nu)
    tau = nuT * (G + np.swapaxes(G, 2, 3)) if form == SYMMETRIC else nuT * G
    tn = (tau * n[:, None, None, :]).sum(axis=3)                                      # [nf, npf, i]
    tnn = (n[:, None, :] * tn).sum(axis=2)
    t = sub(p[:, :, None] * n[:, None, :], tn)
    s = tn + tnn[:, :, None] * n[:, None, :] if ab else -(tn - tnn[:, :, None] * n[:, None, :])
    un = (u * n[:, None, :]).sum(axis=2)
    if ab:
        sm_t, s_t = true["shear_magnitude"], np.abs(true["shear"])
        pos = sm_t > 0
        sm = np.where(pos, (s_t * s).sum(axis=2) / np.where(pos, sm_t, 1), np.sqrt((s * s).sum(axis=2)))
        root = np.sqrt(np.where(pos, sm_t, 1))
        yp = np.where(pos, (sm / (2 * root) * true["d"][:, None] + root * d[:, None]) / nuT, np.sqrt(sm / T(TOL)) * d[:, None] / nuT) if nu > 0 else np.zeros_like(sm)
    else:
        sm = np.sqrt((s * s).sum(axis=2))
        yp = np.sqrt(sm) * d[:, None] / nuT if nu > 0 else np.zeros_like(sm)
    # positions of the face nodes and the nodal rule
    x = np.zeros((nf, npf, dim), dtype=T)
    Xa = np.abs(Xv) if ab else Xv
    for j in range(npf):
        a = loc[:, j]
        vert = a < nv
        li = np.array([PR.LINES[dim][max(int(q) - nv, 0)][0] for q in a])
        lj = np.array([PR.LINES[dim][max(int(q) - nv, 0)][1] for q in a])
        mid = T(0.5) * (Xa[np.arange(nf), li] + Xa[np.arange(nf), lj])
        x[:, j] = np.where(vert[:, None], Xa[np.arange(nf), np.minimum(a, nv - 1)], mid)
    cen = np.abs(np.asarray(centre, dtype=T)) if ab else np.asarray(centre, dtype=T)
    r = sub(x, cen[None, None, :])
    if dim == 2:
        w = area[:, None] * np.array([T(1) / T(6), T(1) / T(6), T(4) / T(6)], dtype=T)[None, :]
        rule = [0, 1, 2]
        cross = sub(r[:, :, 0] * t[:, :, 1], r[:, :, 1] * t[:, :, 0])[:, :, None]
    else:
        w = np.repeat((area * (T(1) / T(3)))[:, None], npf, axis=1)
        rule = [3, 4, 5]
        cross = np.stack([sub(r[:, :, 1] * t[:, :, 2], r[:, :, 2] * t[:, :, 1]), sub(r[:, :, 2] * t[:, :, 0], r[:, :, 0] * t[:, :, 2]),
                          sub(r[:, :, 0] * t[:, :, 1], r[:, :, 1] * t[:, :, 0])], axis=2)
    terms = {"force_pressure": w[:, :, None] * (p[:, :, None] * n[:, None, :]), "force_viscous": w[:, :, None] * (tn if ab else -tn),
             "torque": w[:, :, None] * cross, "flux": w * un, "pressure_integral": w * p}
    contrib = {"area": area}
    for key, v in terms.items():
        acc = v[:, rule[0]]
        for j in rule[1:]:                                                            # in the order of the face nodes
            acc = acc + v[:, j]
        contrib[key] = acc
    return {"det": det, "len": length, "d": d, "area": area, "n": n, "G": G, "pressure": p[:, :, None], "traction": t, "shear": s,
            "shear_magnitude": sm, "normal": np.repeat(n[:, None, :], npf, axis=1), "yplus": yp, "contrib": contrib, "x": x}


def fold_depth(count):
    """additions on the way of one entry through the library's tree over `count` entries: 6 per level of 64"""
    levels = 1
    while count > FOLD:
        count = -(-count // FOLD)
        levels += 1
    return 6 * levels


def fold_tree(v):
    """the library's fold of v [n, ...] over axis 0 in v's own type: blocks of 64 consecutive entries, lane i takes entry i (0 behind the
    end), then lane i += lane i + o for o = 32, 16, ..., 1; level by level until one entry is left (no entry: 0)"""
    v = np.asarray(v)
    if len(v) == 0:
        return np.zeros(v.shape[1:], dtype=v.dtype)
    while True:
        nb = -(-len(v) // FOLD)
        pad = np.zeros((nb * FOLD,) + v.shape[1:], dtype=v.dtype)
        pad[:len(v)] = v
        pad = pad.reshape((nb, FOLD) + v.shape[1:])
        o = FOLD // 2
        while o > 0:
            pad[:, :o] = pad[:, :o] + pad[:, o:2 * o]
            o //= 2
        v = pad[:, 0]
        if nb == 1:
            return v[0]


def _recover(ev, lay, n_groups, groups, T, true=None):
    """area-weighted recovery at the surface nodes, faces in ascending position, both sums folded left to right"""
    ab = true is not None
    ns = len(lay["nodes"])
    fn = lay["face_nodes"]
    dim = ev["n"].shape[1]
    num = {k: np.zeros((ns, ev[k].shape[2]), dtype=T) for k in ("pressure", "traction", "shear")}
    nn, den = np.zeros((ns, dim), dtype=T), np.zeros(ns, dtype=T)
    for f in range(len(fn)):                                                          # the nodes of one face are distinct
        s = fn[f]
        for k in num:
            num[k][s] += ev["area"][f] * ev[k][f]
        nn[s] += ev["area"][f] * ev["n"][f][None, :]
        den[s] += ev["area"][f]
    if ab:
        den = true["_den"]
    out = {k: v / den[:, None] for k, v in num.items()}
    if ab:
        sm_t, s_t = true["shear_magnitude"][:, 0], np.abs(true["shear"])
        pos = sm_t > 0
        out["shear_magnitude"] = np.where(pos, (s_t * out["shear"]).sum(axis=1) / np.where(pos, sm_t, 1), np.sqrt((out["shear"] ** 2).sum(axis=1)))[:, None]
        out["normal"] = nn / true["_nlen"][:, None]
    else:
        out["shear_magnitude"] = np.sqrt((out["shear"] ** 2).sum(axis=1))[:, None]
        nlen = np.sqrt((nn * nn).sum(axis=1))
        out["normal"] = nn / nlen[:, None]
        out["_den"], out["_nlen"] = den, nlen
    return out


def surface(mesh, dofs, solution, cells, lfs, groups=None, n_groups=None, nu=1e-3, form=SYMMETRIC, centre=None):
    """dict:
    layout                 nodes, node_groups, face_nodes, local_nodes (surface())
    areas [nf] (areas_X: their absolute-term sums), G [nf][npf][dim][dim], x [nf][npf][dim]                                                float64 from long double
    faces / nodes          {field: [nf][npf][nc] / [n_s][nc]} float64 from long double; FIELDS / NODE_FIELDS
    faces64 / nodes64      the plain float64 run in the library's order
    faces_X / nodes_X      the absolute-term sums
    totals / totals64      {name: [n_groups] or [n_groups][dim | 3 | 1]} (torque: 3 in 3D, 1 in 2D); totals_ld before rounding
    totals_A               A of every total; depth [n_groups] additions of the fold; n_faces [n_groups]"""
    dim = mesh.dim
    cells, lfs = np.asarray(cells, dtype=np.int64), np.asarray(lfs, dtype=np.int64)
    groups = np.zeros(len(cells), dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    n_groups = int(groups.max()) + 1 if n_groups is None else n_groups
    centre = np.zeros(dim) if centre is None else np.asarray(centre, dtype=np.float64)
    lay = layout(dofs, cells, lfs, groups)
    Xv = np.asarray(mesh.vertices, dtype=np.float64)[np.asarray(mesh.cells)[cells]]   # [nf, nv, dim]
    U = R.cell_velocities(dofs, solution)[cells]
    cd = np.asarray(dofs.cell_dofs)[cells]
    P = np.asarray(solution, dtype=np.float64)[cd[:, [(dim + 1) * v + dim for v in range(dim + 1)]]]
    runs = {}
    for name, T in (("ld", LD), ("f64", np.float64)):
        with np.errstate(invalid="ignore", divide="ignore"):
            ev = _evaluate(dim, Xv, U, P, lfs, nu, form, centre, T)
            runs[name] = (ev, _recover(ev, lay, n_groups, groups, T))
    ev, rec = runs["ld"]
    with np.errstate(invalid="ignore", divide="ignore"):
        evx = _evaluate(dim, Xv, U, P, lfs, nu, form, centre, LD, true=ev)
        recx = _recover(evx, lay, n_groups, groups, LD, true=rec)

    def shaped(v):
        return v[:, :, None] if v.ndim == 2 else v
    out = {"layout": lay, "areas": ev["area"].astype(np.float64), "areas_X": evx["area"].astype(np.float64), "G": ev["G"].astype(np.float64), "x": ev["x"].astype(np.float64),
           "faces": {k: shaped(ev[k]).astype(np.float64) for k in FIELDS}, "faces64": {k: shaped(runs["f64"][0][k]) for k in FIELDS},
           "faces_X": {k: shaped(evx[k]).astype(np.float64) for k in FIELDS},
           "nodes": {k: rec[k].astype(np.float64) for k in NODE_FIELDS}, "nodes64": {k: runs["f64"][1][k] for k in NODE_FIELDS},
           "nodes_X": {k: recx[k].astype(np.float64) for k in NODE_FIELDS}}
    sel = [np.flatnonzero(groups == g) for g in range(n_groups)]                      # ascending position in the caller's list
    out["n_faces"] = np.array([len(s) for s in sel])
    out["depth"] = np.array([fold_depth(len(s)) + 2 for s in sel])
    for key, (e, _) in (("totals_ld", runs["ld"]), ("totals64", runs["f64"]), ("totals_A", (evx, None))):
        out[key] = {k: np.stack([fold_tree(e["contrib"][k][s]) for s in sel]) for k in TOTALS}
    out["totals"] = {k: v.astype(np.float64) for k, v in out["totals_ld"].items()}
    out["totals_A"] = {k: v.astype(np.float64) for k, v in out["totals_A"].items()}
    return out


def total_bound(ref, key):
    """(C1 + depth) 2^-53 A of total `key`, per group (and component)"""
    A = ref["totals_A"][key]
    d = ref["depth"].reshape((-1,) + (1,) * (A.ndim - 1))
    return (C1 + d) * 2.0 ** -53 * A


def field_ratio(got, ref, X):
    """largest |got - ref| / X (0 / 0 = 0: where X vanishes the value has to be exactly 0)"""
    d, X = np.abs(np.asarray(got) - ref), np.asarray(X)
    r = np.where(X > 0, d / np.where(X > 0, X, 1.0), np.where(d == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0
