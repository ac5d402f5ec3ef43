"""Extended-precision restatement of the element assembly of csrc/nsx_assemble.hip and of the face quadrature of csrc/nsx_forces.hip,
the entry-by-entry bound the device results are held to, a float64 restatement with a choice of summation order (the function under
mutation) and its mutants.  Shared by tests/test_assembly_reference.py (CPU) and tests/test_gpu_assembly.py.

Reference.  Plain numpy in np.longdouble (64-bit significand on x86), vectorised over the cells, from the caller's data alone:
dofs.cell_dofs, dofs.cell_coords, the tables, nu, deltat and the solution vector.  Nothing comes from the device or the oracle.
  geometry   J[d][k] = X[k+1][d] - X[0][d], det and the cofactors as csrc/nsx_setup.hip writes them, Ji = cofactor / det, |det|
  blocks     exactly as the headers of k_cell_static and k_cell_convection define them:
             mass/dt      sum_q N_a N_b (1/dt) |det| w_q                      nu K   sum_q nu (J^-T dN_a . J^-T dN_b) |det| w_q
             D[a][v][c]   sum_q psi_v (J^-T dN_a)_c |det| w_q                 Mp/nu  sum_q psi_v psi_u / nu |det| w_q
             C[a][b]      conv_scale sum_q N_a (Ji w_q . dN_b) |det| w_q  (+ sum_q N_a N_b 0.5 (sum_a dN_a . Ji U_a) |det| w_q with Temam)
  assembly   on dofs.reference_sparsity(block) in the padded layout export_block returns, every entry's contributions added in
             ascending cell order; block(0,1) = -sum D, block(1,0) = +sum D; cross-component slots of block(0,0) are structural zeros.

Bound companion (derived, not measured).  With every value v come
  A   the same formula with every factor replaced by its absolute value: |table values|, the sums of |cofactor terms| over |det| in
      place of Ji, |u|, the weights; carried through the gather as a plain sum.  (A is computed by calling the same code on those
      inputs.)
  n   the roundings along the longest dependency path of the kernel's loop nest, a sum of m terms counted as m additions
      (D = dim, P = n_p2, Q = n_q, L = length of the entry's gather list):
        mass     3 products + (|det| w) + fl(1/dt) + Q                                                       = Q + 5
        nu K     ga: D, gb: D, ga gb: 1, sum over d: D, nu gg (|det| w): 3, sum over q: Q                    = 3 D + 4 + Q
        D        ga: D, psi ga (|det| w): 3, Q                                                               = D + 3 + Q
        Mp/nu    psi psi / nu (|det| w): 4, Q                                                                = Q + 4
        C        Ut: D; wt: 1 + P; what = wt (jxw cs): 3         -> what: D + P + 4
                 div: Ut D, product 1, sum P D; tq = 0.5 div jxw: 2 (the 0.5 is exact, jxw is one)  -> tq: D + P D + 3
                 g: max(what, tq) + 1 product + D (+ 1 with Temam);  out: 1 product + Q
                 no Temam: 2 D + P + Q + 6         Temam: 2 D + P D + Q + 6
        gather   L additions (the multiplication by sign = +-1 is exact), + 1 where a base is added
        system(0,0) = (M + K) + C and S0 + C_new: the largest n of the three + 2;  A = A_M + A_K + A_C
        rhs      (M/dt) u_n by rows: n_M of the row's entries + row length + 1 product;  A_i = sum_j A_M,ij |u_j|
  n_g the roundings of the host geometry (csrc/nsx_setup.hip), per geometry factor of a term, g = 5 in 2D and 12 in 3D:
        2D  J entries 1, det = 2 products - : 3 kappa;  Ji = +-J / det: 1 + 1 + 3 kappa                      <= 5 kappa
        3D  det: 3 J entries, 2 products, 2 additions: 7 kappa;  cofactor 2 J + product + difference: 4 (against the sum of its
            |terms|, which is what A carries); division 1                                                    <= 12 kappa
      a term has 1 (mass, Mp), 2 (D, C: one Ji and |det|) or 3 (K: two Ji and |det|) geometry factors: n_g = factors x g.
  kappa_c  per cell, the largest of sum|terms| / |value| over the determinant and every non-zero cofactor as written in
           csrc/nsx_setup.hip (a cofactor that is exactly 0 has its error covered by A, which carries the sum of its |terms|).
           For an assembled entry: the largest over its contributing cells.
The bound is    |dev - ref| <= (n + n_g kappa) 2^-53 A    for every stored entry, and exactly 0 where A = 0.
It holds for any summation order and wherever the compiler contracts a product and a sum into an FMA (Higham, Accuracy and Stability,
sections 3.1 / 4.2).  The reference's own error is 2^-11 of it and is not added.

Forces (k_forces).  Per (face, point) the two formulas of the kernel; A with |nref|, |Ji| sums, |dN|, |u|, |psi|, |p| and the TRUE
len = |J^-T nref| and t2 = nx^2 + ny^2 (sums of squares: no cancellation; their absolute-valued versions would be larger and would
make A smaller).  n: nv D, len 2 D + 2, n = nv / len: 3 D + 3; p: n_p1 + 1; G: D + 1 + P; jxw: 2 D + 5
  2D  (nu G - p) n summed over j, times jxw: 7 D + P + 13      3D  n G tang / t2 summed over i, j, rho nu s n - p n, times jxw: 18 D + D^2 + P + 31
n_g = 8 g (n twice through nv and len, |det|, len, Ji in G, and in 3D tang and t2).  Only the two sums are observable:
bound = sum of the per-point bounds + (n_faces n_qf) 2^-53 (sum |contribution| + sum of the per-point bounds).

Tables.  tables_from_points evaluates the P2 / P1 shape functions in the front end's local order (vertices, then TRI_LINES /
TET_LINES) in long double and rounds once.  The kernels' contract is "any tables": synthetic_rule gives seeded points strictly
inside the simplex with positive weights normalised to the reference volume -- what is tested with them is ARITHMETIC, not
quadrature exactness.  The normalisation keeps "the mass sums to dim |Omega| / dt" and "stiffness rows sum to 0" true (both only
need sum_a N_a = 1 and sum_q w_q = |ref|).  gauss_rule_ld is a conical rule built in long double (4 Gauss-Legendre points per
direction, exact for the degree-5 integrands of the P2 blocks): the closed forms of tests/golden are reproduced with it.

Mutants of the float64 restatement (restate(..., mutant=...)): MUTANTS below."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TRI_LINES = ((0, 1), (1, 2), (2, 0))
TET_LINES = ((0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3))
# the (dim, n_q) cases of dispatch_conv (csrc/nsx_assemble.hip); tests/test_assembly_reference.py keeps the list in sync
INSTANTIATIONS = ((2, 3), (2, 4), (2, 6), (2, 7), (2, 12), (3, 4), (3, 10), (3, 11), (3, 14), (3, 15), (3, 24))
TEMAM, DOUBLE_CONVECTION = 1, 2
ORDERS = ("kernel", "reversed", "pairwise")
MUTANTS = ("lost_half", "signed_det", "swapped_ji", "weight", "gather_tail", "conv_scale", "dbar_own", "normal")
G_FACTOR = {2: 5, 3: 12}


# ------------------------------------------------------------------------------------------------------------------ sums
def acc(terms, order="kernel"):
    """sum of a list of arrays in the given order"""
    terms = list(terms)
    if order == "reversed":
        terms = terms[::-1]
    if order == "pairwise":
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


# ------------------------------------------------------------------------------------------------------------------ tables
class TablesLike:
    """the fields Nsx.__init__ reads"""

    def __init__(self, dim, points, weights, N2, dN2, N1):
        self.dim, self.points, self.weights, self.N2, self.dN2, self.N1 = dim, points, weights, N2, dN2, N1
        self.n_q, self.n_p2, self.n_p1 = len(weights), N2.shape[1], N1.shape[1]


def tables_from_points(dim, points, weights, rounded=True):
    """P2 / P1 shape tables at `points` [n_q][dim] of the reference simplex, evaluated in long double; rounded once to float64
    (rounded = False keeps long double: the closed-form test)"""
    x = np.asarray(points, dtype=LD).reshape(-1, dim)
    nq, nv = len(x), dim + 1
    lam = np.concatenate([(LD(1) - x.sum(axis=1))[:, None], x], axis=1)                    # [q][v]
    dl = np.concatenate([-np.ones((1, dim), dtype=LD), np.eye(dim, dtype=LD)], axis=0)      # [v][k]
    lines = TRI_LINES if dim == 2 else TET_LINES
    np2 = nv + len(lines)
    N2, dN2 = np.zeros((nq, np2), dtype=LD), np.zeros((nq, np2, dim), dtype=LD)
    for v in range(nv):
        N2[:, v] = lam[:, v] * (2 * lam[:, v] - 1)
        dN2[:, v, :] = (4 * lam[:, v] - 1)[:, None] * dl[v][None, :]
    for l, (a, b) in enumerate(lines):
        N2[:, nv + l] = 4 * lam[:, a] * lam[:, b]
        dN2[:, nv + l, :] = 4 * (lam[:, a, None] * dl[b][None, :] + lam[:, b, None] * dl[a][None, :])
    w = np.asarray(weights, dtype=LD)
    out = (x, w, N2, dN2, lam)
    if rounded:
        out = tuple(np.ascontiguousarray(a.astype(np.float64)) for a in out)
    return TablesLike(dim, *out)


def synthetic_rule(dim, n_q, seed=2026):
    """seeded points strictly inside the reference simplex, positive weights summing to its volume (float64 data)"""
    rng = np.random.default_rng(seed + 100 * dim + n_q)
    lam = rng.dirichlet(np.full(dim + 1, 2.0), size=n_q)
    lam = np.clip(lam, 0.02, None)
    lam /= lam.sum(axis=1)[:, None]
    w = rng.uniform(0.5, 1.5, size=n_q)
    w *= (0.5 if dim == 2 else 1.0 / 6.0) / w.sum()
    return lam[:, 1:].copy(), w


def gauss_rule_ld(dim, n=4):
    """conical (Duffy) product of n-point Gauss-Legendre rules on [0, 1], nodes Newton-refined and weights formed in long double"""
    x = np.polynomial.legendre.leggauss(n)[0].astype(LD)
    for _ in range(3):
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x.copy()
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    dp = n * (x * p1 - p0) / (x * x - 1)
    w = 2 / ((1 - x * x) * dp * dp) / 2
    t = (x + 1) / 2
    pts, wts = [], []
    if dim == 2:
        for i in range(n):
            for j in range(n):
                pts.append([t[i], t[j] * (1 - t[i])])
                wts.append(w[i] * w[j] * (1 - t[i]))
    else:
        for i in range(n):
            for j in range(n):
                for k in range(n):
                    pts.append([t[i], t[j] * (1 - t[i]), t[k] * (1 - t[i]) * (1 - t[j])])
                    wts.append(w[i] * w[j] * w[k] * (1 - t[i]) ** 2 * (1 - t[j]))
    return np.array(pts, dtype=LD), np.array(wts, dtype=LD)


def rule(dim, n_q):
    """the tables the GPU test runs instantiation (dim, n_q) with: the front end's own rule where it makes one, else a synthetic one"""
    from navierstokes_project_nm4pde_amd.frontend import Tables
    if (dim, n_q) in ((2, 7), (3, 14)):
        t = Tables(dim)
    elif (dim, n_q) == (2, 4):
        t = Tables(2, Tables.HIGH, 2)
    else:
        return tables_from_points(dim, *synthetic_rule(dim, n_q))
    assert t.n_q == n_q
    return t


def abs_tables(t, dtype=LD):
    return TablesLike(t.dim, None, np.abs(np.asarray(t.weights, dtype=dtype)), np.abs(np.asarray(t.N2, dtype=dtype)),
                      np.abs(np.asarray(t.dN2, dtype=dtype)), np.abs(np.asarray(t.N1, dtype=dtype)))


def cast_tables(t, dtype):
    return TablesLike(t.dim, None, *(np.asarray(a, dtype=dtype) for a in (t.weights, t.N2, t.dN2, t.N1)))


# ------------------------------------------------------------------------------------------------------------------ geometry
class Geometry:
    """dim, Ji, absJi, det, adet, kappa of every cell"""


def geometry(cell_coords, dtype=LD):
    """Ji [c][k][d], det (signed), adet, absJi (sum of |cofactor terms| / |det|), kappa -- formulas as in csrc/nsx_setup.hip"""
    X = np.asarray(cell_coords, dtype=dtype)
    nc, nv, dim = X.shape
    J = [[X[:, k + 1, d] - X[:, 0, d] for k in range(dim)] for d in range(dim)]          # J[d][k]
    if dim == 2:
        dt_terms = [J[0][0] * J[1][1], -(J[0][1] * J[1][0])]
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        cof = [[[J[1][1]], [-J[0][1]]], [[-J[1][0]], [J[0][0]]]]
    else:
        def m2(a, b, c, d):
            return [J[a[0]][a[1]] * J[b[0]][b[1]], -(J[c[0]][c[1]] * J[d[0]][d[1]])]
        i0, i1, i2 = m2((1, 1), (2, 2), (1, 2), (2, 1)), m2((1, 0), (2, 2), (1, 2), (2, 0)), m2((1, 0), (2, 1), (1, 1), (2, 0))
        dt_terms = [J[0][0] * i0[0], J[0][0] * i0[1], -(J[0][1] * i1[0]), -(J[0][1] * i1[1]), J[0][2] * i2[0], J[0][2] * i2[1]]
        det = J[0][0] * (i0[0] + i0[1]) - J[0][1] * (i1[0] + i1[1]) + J[0][2] * (i2[0] + i2[1])
        cof = [[m2((1, 1), (2, 2), (1, 2), (2, 1)), m2((0, 2), (2, 1), (0, 1), (2, 2)), m2((0, 1), (1, 2), (0, 2), (1, 1))],
               [m2((1, 2), (2, 0), (1, 0), (2, 2)), m2((0, 0), (2, 2), (0, 2), (2, 0)), m2((0, 2), (1, 0), (0, 0), (1, 2))],
               [m2((1, 0), (2, 1), (1, 1), (2, 0)), m2((0, 1), (2, 0), (0, 0), (2, 1)), m2((0, 0), (1, 1), (0, 1), (1, 0))]]
    g = Geometry()
    g.dim, g.det, g.adet = dim, det, np.abs(det)
    g.Ji, g.absJi = np.zeros((nc, dim, dim), dtype=dtype), np.zeros((nc, dim, dim), dtype=dtype)
    kap = sum(np.abs(t) for t in dt_terms) / np.abs(det)
    for k in range(dim):
        for d in range(dim):
            val, s = sum(cof[k][d]), sum(np.abs(t) for t in cof[k][d])
            g.Ji[:, k, d], g.absJi[:, k, d] = val / det, s / np.abs(det)
            with np.errstate(divide="ignore", invalid="ignore"):
                kap = np.maximum(kap, np.where(val != 0, s / np.abs(np.where(val != 0, val, 1)), 1))
    g.kappa = kap
    return g


# ------------------------------------------------------------------------------------------------------------------ element blocks
def static_blocks(Ji, adet, t, nu, deltat, order="kernel"):
    """mass/dt [c][a][b], nu K [c][a][b], D [c][a][v][cc], Mp/nu [c][v][u] in the dtype of the inputs, products associated as in
    k_cell_static"""
    dtype = Ji.dtype.type
    nc, dim = Ji.shape[0], Ji.shape[1]
    nq = len(t.weights)
    inv_dt, nu = dtype(1) / dtype(deltat), dtype(nu)
    mass, stiff, D, pm = [], [], [], []
    for q in range(nq):
        jxw = adet * t.weights[q]                                                       # [c]
        N, N1 = t.N2[q], t.N1[q]
        mass.append((N[:, None] * N[None, :] * inv_dt)[None] * jxw[:, None, None])
        # ga[c][a][d] = sum_k Ji[c][k][d] dN[a][k]
        ga = acc([Ji[:, None, k, :] * t.dN2[q][None, :, k, None] for k in range(dim)], order)
        gg = acc([ga[:, :, None, d] * ga[:, None, :, d] for d in range(dim)], order)
        stiff.append(nu * gg * jxw[:, None, None])
        D.append(N1[None, None, :, None] * ga[:, :, None, :] * jxw[:, None, None, None])
        pm.append((N1[:, None] * N1[None, :] / nu)[None] * jxw[:, None, None])
    return acc(mass, order), acc(stiff, order), acc(D, order), acc(pm, order)


def convection_block(Ji, adet, t, u, temam, conv_scale, order="kernel", half=0.5):
    """C [c][a][b] as k_cell_convection computes it; u [c][a][d] the cell's velocity values"""
    dtype = Ji.dtype.type
    nc, dim = Ji.shape[0], Ji.shape[1]
    nq, np2 = len(t.weights), t.N2.shape[1]
    Ut = acc([Ji[:, None, :, d] * u[:, :, None, d] for d in range(dim)], order)        # [c][a][k]
    cols = []
    for q in range(nq):
        jxw = adet * t.weights[q]
        wt = acc([Ut[:, a, :] * t.N2[q, a] for a in range(np2)], order)                # [c][k]
        what = wt * (jxw * dtype(conv_scale))[:, None]
        g = [what[:, None, k] * t.dN2[q][None, :, k] for k in range(dim)]             # [c][b]
        if temam:
            div = acc([t.dN2[q, a, k] * Ut[:, a, k] for a in range(np2) for k in range(dim)], order)
            g.append(t.N2[q][None, :] * (dtype(half) * div * jxw)[:, None])
        cols.append(t.N2[q][None, :, None] * acc(g, order)[:, None, :])                # [c][a][b]
    return acc(cols, order)


def counts(dim, n_q, temam):
    """n of the module docstring for (mass, stiffness, D, pmass, convection)"""
    P = 6 if dim == 2 else 10
    return {"mass": n_q + 5, "stiff": 3 * dim + 4 + n_q, "D": dim + 3 + n_q, "pmass": n_q + 4,
            "conv": 2 * dim + (P * dim if temam else P) + n_q + 6}


GEO_FACTORS = {"mass": 1, "stiff": 3, "D": 2, "pmass": 1, "conv": 2}


# ------------------------------------------------------------------------------------------------------------------ topology
class Topology:
    """cell -> node tables, scalar graphs and their maps into the padded reference graphs, gather positions"""

    def __init__(self, dofs):
        dim = self.dim = dofs.dim
        nv = dim + 1
        cd = np.asarray(dofs.cell_dofs, dtype=np.int64)
        self.n_cells, self.n_u, self.n_p = cd.shape[0], dofs.n_u, dofs.n_p
        self.np2 = 6 if dim == 2 else 10
        base = [(dim + 1) * a if a < nv else nv * (dim + 1) + dim * (a - nv) for a in range(self.np2)]
        self.c2 = cd[:, base] // dim                                                        # [c][a] P2 node
        self.c1 = cd[:, [(dim + 1) * v + dim for v in range(nv)]] - dofs.n_u                # [c][v] P1 node
        self.N2, self.NP = dofs.n_u // dim, dofs.n_p
        self.padded = {b: tuple(np.asarray(a, dtype=np.int64) for a in dofs.reference_sparsity(b)) for b in range(4)}
        self.graph, self.pad_map, self.pad_comp = {}, {}, {}
        for b in range(4):
            rp, ci = self.padded[b]
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
            rn, rc = (rows // dim, rows % dim) if b in (0, 1) else (rows, np.zeros_like(rows))
            cn, cc = (ci // dim, ci % dim) if b in (0, 2) else (ci, np.zeros_like(ci))
            ncol = self.N2 if b in (0, 2) else self.NP
            key = rn * ncol + cn
            skeys = np.unique(key[(rc == 0) & (cc == 0)])                                   # the scalar graph, sorted by (row, col)
            pos = np.searchsorted(skeys, key)
            assert np.all(skeys[np.minimum(pos, len(skeys) - 1)] == key)
            self.graph[b] = (skeys, ncol)
            if b == 0:
                self.pad_map[b], self.pad_comp[b] = np.where(rc == cc, pos, -1), np.zeros_like(pos)
            else:
                self.pad_map[b], self.pad_comp[b] = pos, (rc if b == 1 else cc)
        r2, r1 = self.c2, self.c1
        self.epos = {0: self._epos(0, r2[:, :, None], r2[:, None, :]), 1: self._epos(1, r2[:, :, None], r1[:, None, :]),
                     2: self._epos(2, r1[:, :, None], r2[:, None, :]), 3: self._epos(3, r1[:, :, None], r1[:, None, :])}
        # scalar block(0,0) graph as CSR (rhs) and its diagonal
        sk, ncol = self.graph[0]
        self.A_rows, self.A_cols = sk // ncol, sk % ncol
        self.A_diag = np.searchsorted(sk, np.arange(self.N2) * ncol + np.arange(self.N2))

    def _epos(self, b, rn, cn):
        skeys, ncol = self.graph[b]
        key = (rn * ncol + cn).reshape(self.n_cells, -1)
        pos = np.searchsorted(skeys, key)
        assert np.all(skeys[pos] == key)
        return pos                                                                          # [c][local pair] -> scalar entry

    def gather_matrix(self, b, vals, fill=0):
        """[entry][k-th contribution, ascending cell][...] padded with `fill`, and the list lengths L"""
        pos = self.epos[b]
        nc, m = pos.shape
        vals = vals.reshape(nc, m, -1)
        e = pos.reshape(-1)
        order = np.argsort(e, kind="stable")                                                # cell-major input: ascending cell inside an entry
        es = e[order]
        n_out = len(self.graph[b][0])
        L = np.bincount(es, minlength=n_out)
        start = np.concatenate([[0], np.cumsum(L)])[:-1]
        rank = np.arange(len(es)) - start[es]
        M = np.full((n_out, int(L.max()), vals.shape[2]), fill, dtype=vals.dtype)
        M[es, rank] = vals.reshape(-1, vals.shape[2])[order]
        return M, L

    def to_padded(self, b, scalar):
        """scalar [entry][comp] -> values on the padded graph of block b"""
        pm, pc = self.pad_map[b], self.pad_comp[b]
        out = scalar[np.maximum(pm, 0), pc]
        return np.where(pm >= 0, out, scalar.dtype.type(0))


def gather(topo, b, vals, order="kernel", drop_tail=False):
    """sum of every entry's contributions (vals [c][pairs...] of block b's element block) -> [entry][comp]"""
    M, L = topo.gather_matrix(b, vals)
    if drop_tail:                                   # mutant: the last contribution of the lists whose length is no multiple of 4
        bad = np.nonzero(L % 4 != 0)[0]
        M[bad, L[bad] - 1] = 0
    if order == "reversed":                         # zeros of the padding are exact: move them in front instead of reversing inside L
        return acc([M[:, k] for k in range(M.shape[1])][::-1], "kernel"), L
    return acc([M[:, k] for k in range(M.shape[1])], order), L


def cell_values(topo, x):
    """u [c][a][d] of the block vector x"""
    xu = np.asarray(x)[:topo.n_u].reshape(topo.N2, topo.dim)
    return xu[topo.c2]


# ------------------------------------------------------------------------------------------------------------------ values with bounds
class Val:
    """v (long double), A, n, kappa, n_g of every entry"""

    def __init__(self, v, A, n, kappa, ng):
        self.v, self.A = v, A
        self.n, self.kappa, self.ng = (np.broadcast_to(np.asarray(a), v.shape) for a in (n, kappa, ng))

    def bound(self):
        return (self.n.astype(LD) + self.ng.astype(LD) * self.kappa.astype(LD)) * LD(U) * self.A

    def check(self, dev, name=""):
        """(messages, largest error / bound): every entry within the bound, exactly 0 where A = 0"""
        dev = np.asarray(dev, dtype=np.float64)
        assert dev.shape == self.v.shape, (name, dev.shape, self.v.shape)
        err, b = np.abs(dev.astype(LD) - self.v), self.bound()
        msgs = []
        zero = self.A == 0
        if np.any(dev[zero] != 0.0):
            msgs.append("%s: %d entries with A = 0 are not exactly 0" % (name, int(np.count_nonzero(dev[zero] != 0.0))))
        bad = np.nonzero(~zero & ~(err <= b))[0]
        if len(bad):
            k = bad[np.argmax((err[bad] / b[bad]).astype(np.float64))]
            msgs.append("%s: %d entries outside the bound, worst entry %d: %.17g against %.17g, error %.3g = %.3g x bound" %
                        (name, len(bad), k, dev[k], float(self.v[k]), float(err[k]), float(err[k] / b[k])))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(zero, 0, err / np.where(zero, 1, b))
        return msgs, float(ratio.max()) if len(ratio) else 0.0


def _combine(vals, extra):
    return Val(sum(x.v for x in vals), sum(x.A for x in vals), np.max([x.n for x in vals], axis=0) + extra,
               np.max([x.kappa for x in vals], axis=0), np.max([x.ng for x in vals], axis=0))


class Reference:
    """the extended-precision assembly of one (dofs, tables, nu, deltat)"""

    def __init__(self, dofs, tables, nu, deltat, topo=None, coords=None):
        self.dofs, self.dim = dofs, dofs.dim
        self._kap = {}
        self.topo = topo or Topology(dofs)
        self.t, self.ta = cast_tables(tables, LD), abs_tables(tables)
        self.n_q = len(self.t.weights)
        self.nu, self.deltat = LD(nu), LD(deltat)
        self.geo = geometry(dofs.cell_coords if coords is None else coords)
        g = self.geo
        self.static = self._assemble_static(static_blocks(g.Ji, g.adet, self.t, self.nu, self.deltat),
                                            static_blocks(g.absJi, g.adet, self.ta, self.nu, self.deltat))

    def _val(self, b, name, el, elA, temam=False, sign=1):
        topo, g = self.topo, self.geo
        v, L = gather(topo, b, el)
        A, _ = gather(topo, b, elA)
        if b not in self._kap:                      # the largest kappa over an entry's contributing cells: geometry alone
            K, _ = topo.gather_matrix(b, np.broadcast_to(g.kappa.reshape((-1,) + (1,) * (el.ndim - 1)), el.shape).copy(), fill=0)
            self._kap[b] = K.max(axis=1)
        kap = self._kap[b]
        n = counts(self.dim, self.n_q, temam)[name] + L
        ng = GEO_FACTORS[name] * G_FACTOR[self.dim]
        pad = lambda s: topo.to_padded(b, s)
        return Val(sign * pad(v), pad(A), pad(np.repeat(n[:, None], v.shape[1], 1)), pad(kap), ng)

    def _assemble_static(self, el, elA):
        mass, stiff, D, pm = el
        massA, stiffA, DA, pmA = elA
        Dt, DtA = np.transpose(D, (0, 2, 1, 3)), np.transpose(DA, (0, 2, 1, 3))             # [c][v][a][cc]: block(1,0) pairs (v, a)
        return {"mass": self._val(0, "mass", mass, massA), "stiff": self._val(0, "stiff", stiff, stiffA),
                "G": self._val(1, "D", D, DA, sign=-1), "B": self._val(2, "D", Dt, DtA), "pmass": self._val(3, "pmass", pm, pmA)}

    def convection(self, x, flags=0, first=True):
        g, topo = self.geo, self.topo
        temam = bool(flags & TEMAM)
        cs = 2 if (first and flags & DOUBLE_CONVECTION) else 1
        u = cell_values(topo, np.asarray(x, dtype=LD))
        return self._val(0, "conv", convection_block(g.Ji, g.adet, self.t, u, temam, cs), convection_block(g.absJi, g.adet, self.ta, np.abs(u), temam, cs), temam)

    def state(self, x, flags=0, first=True):
        """everything assemble (first) / assemble_time_step leaves: dict of Val on the padded graphs, rhs over the block vector"""
        s = dict(self.static)
        s["conv"] = self.convection(x, flags, first)
        s["F"] = _combine([s["mass"], s["stiff"], s["conv"]], 2)
        s["rhs"] = self.rhs(x)
        return s

    def rhs(self, x):
        topo, dim = self.topo, self.dim
        m = self.static["mass"]
        rp, ci = topo.padded[0]
        xl = np.asarray(x, dtype=LD)
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        same = (rows % dim) == (ci % dim)
        n_u = topo.n_u
        v, A = np.zeros(len(xl), dtype=LD), np.zeros(len(xl), dtype=LD)
        n, kap = np.zeros(len(xl), dtype=np.int64), np.ones(len(xl), dtype=LD)
        np.add.at(v, rows[same], (m.v * xl[ci])[same])
        np.add.at(A, rows[same], (m.A * np.abs(xl[ci]))[same])
        cnt = np.bincount(rows[same], minlength=n_u)
        nmax = np.zeros(n_u, dtype=np.int64)
        np.maximum.at(nmax, rows[same], m.n[same])
        n[:n_u] = nmax + cnt + 1
        np.maximum.at(kap, rows[same], m.kappa[same].astype(LD))
        return Val(v, A, n, kap, GEO_FACTORS["mass"] * G_FACTOR[dim])


# ------------------------------------------------------------------------------------------------------------------ exact operations
def rank_nodes_default(dofs):
    ptr = np.asarray(dofs.owned_u_ptr)
    return [np.arange(ptr[r], ptr[r + 1]) for r in range(len(ptr) - 1)]


def apply_boundary_values(topo, F, G, rhs, sol, bd, bv, rank_nodes, dbar_own=False):
    """MatrixTools::apply_boundary_values as run_dirichlet does it, on values in the padded layout (any dtype; exact operations but
    for value * dbar): returns new (F, G, rhs, sol, dbar per rank).  rank_nodes: for every rank the caller's P2 nodes of its row
    range, in the order of the rows."""
    dim = topo.dim
    F, G, rhs, sol = (np.array(a, copy=True) for a in (F, G, rhs, sol))
    rp, ci = topo.padded[0]
    grp = topo.padded[1][0]
    diag = np.array([rp[i] + int(np.nonzero(ci[rp[i]:rp[i + 1]] == i)[0][0]) for i in range(0, topo.n_u, dim)])     # of component 0
    dbar, node_rank = [], np.zeros(topo.N2, dtype=np.int64)
    for r, nodes in enumerate(rank_nodes):
        node_rank[nodes] = r
        d = F.dtype.type(1)
        for v in F[diag[nodes]]:
            if v != 0:
                d = abs(v)
                break
        dbar.append(d)
    for dof, val in zip(np.asarray(bd, dtype=np.int64), np.asarray(bv)):
        node = dof // dim
        d = abs(F[diag[node]]) if dbar_own else dbar[node_rank[node]]
        row = slice(rp[dof], rp[dof + 1])
        F[row] = np.where(ci[row] == dof, d, 0)
        G[grp[dof]:grp[dof + 1]] = 0
        rhs[dof] = F.dtype.type(val) * d
        sol[dof] = val
    return F, G, rhs, sol, dbar


def add_rhs(rhs, dofs_, vals):
    out = np.array(rhs, copy=True)
    out[np.asarray(dofs_, dtype=np.int64)] += np.asarray(vals, dtype=out.dtype)
    return out


# ------------------------------------------------------------------------------------------------------------------ forces
NREF = {2: ((0, -1), (1, 1), (-1, 0)), 3: ((0, 0, -1), (0, -1, 0), (-1, 0, 0), (1, 1, 1))}


def force_counts(dim):
    P = 6 if dim == 2 else 10
    return (7 * dim + P + 13) if dim == 2 else (18 * dim + dim * dim + P + 31)


def forces_points(topo, geo, ftab, x, cells, lfaces, nu, dtype=LD, absolute=False, flip_face=None, order="kernel"):
    """(drag, lift) [face][point] by the two formulas of k_forces.  absolute: the A companion (see the module docstring).
    Also returns nx^2 + ny^2 (3D) of every face."""
    dim = topo.dim
    cells, lfaces = np.asarray(cells, dtype=np.int64), np.asarray(lfaces, dtype=np.int64)
    nf, nqf = len(cells), ftab.n_qf
    np2, np1 = topo.np2, dim + 1
    f = lambda a: np.abs(np.asarray(a, dtype=dtype)) if absolute else np.asarray(a, dtype=dtype)
    dN2f, N1f = f(np.asarray(ftab.dN2).reshape(-1, np2, dim)), f(np.asarray(ftab.N1).reshape(-1, np1))     # rows [local face][point]
    wf = np.asarray(ftab.weights[:nqf], dtype=dtype)
    xs = np.asarray(x, dtype=dtype)
    Ji_true, adet = geo.Ji[cells].astype(dtype), geo.adet[cells].astype(dtype)
    Ji = geo.absJi[cells].astype(dtype) if absolute else Ji_true
    nref = np.array(NREF[dim], dtype=dtype)[lfaces]                                        # [f][k]
    if flip_face is not None:
        nref = np.where((lfaces == flip_face)[:, None], -nref, nref)
    mref = dtype(0.5 if dim == 3 else 1.0)
    nv_true = acc([Ji_true[:, k, :] * nref[:, k, None] for k in range(dim)], order)
    ln = np.sqrt(acc([nv_true[:, d] * nv_true[:, d] for d in range(dim)], order))
    n_true = -nv_true / ln[:, None]
    n = acc([Ji[:, k, :] * np.abs(nref[:, k, None]) for k in range(dim)], order) / ln[:, None] if absolute else n_true
    t2 = n_true[:, 1] * n_true[:, 1] + n_true[:, 0] * n_true[:, 0]
    u = f(xs[:topo.n_u].reshape(-1, dim)[topo.c2[cells]])                                  # [f][a][i]
    pn = f(xs[topo.n_u + topo.c1[cells]])                                                  # [f][v]
    nu = dtype(nu)
    drag, lift = np.zeros((nf, nqf), dtype=dtype), np.zeros((nf, nqf), dtype=dtype)
    for q in range(nqf):
        tq = lfaces * nqf + q
        jxw = wf[q] * adet * ln * mref
        p = acc([N1f[tq, v] * pn[:, v] for v in range(np1)], order)
        g = [acc([Ji[:, k, :] * dN2f[tq, a, k, None] for k in range(dim)], order) for a in range(np2)]     # [a] -> [f][j]
        G = acc([u[:, a, :, None] * g[a][:, None, :] for a in range(np2)], order)                          # [f][i][j]
        if dim == 3:
            nx, ny = n[:, 0], n[:, 1]
            tang = [ny, nx if absolute else -nx, np.zeros_like(nx)]
            with np.errstate(divide="ignore", invalid="ignore"):       # t2 = 0: a face the caller leaves out (all_faces)
                s = acc([n[:, i] * G[:, i, j] * (tang[j] / t2) for i in range(3) for j in range(3)], order)
            if absolute:
                drag[:, q], lift[:, q] = (nu * s * ny + p * nx) * jxw, (nu * s * nx + p * ny) * jxw
            else:
                drag[:, q], lift[:, q] = (nu * s * ny - p * nx) * jxw, -(nu * s * nx + p * ny) * jxw
        else:
            for i, out in ((0, drag), (1, lift)):
                terms = [((nu * G[:, i, j] + (p if i == j else 0)) if absolute else (nu * G[:, i, j] - (p if i == j else 0))) * n[:, j] for j in range(2)]
                out[:, q] = acc(terms, order) * jxw
    return drag, lift, t2


def forces(topo, geo, ftab, x, cells, lfaces, nu):
    """((drag, lift) sums in long double, (bound_drag, bound_lift)) -- the bound of the module docstring"""
    d, l, _ = forces_points(topo, geo, ftab, x, cells, lfaces, nu)
    if d.size == 0:
        return (LD(0), LD(0)), (LD(0), LD(0))
    dA, lA, _ = forces_points(topo, geo, ftab, x, cells, lfaces, nu, absolute=True)
    dim = topo.dim
    fac = (LD(force_counts(dim)) + 8 * G_FACTOR[dim] * geo.kappa[np.asarray(cells, dtype=np.int64)].astype(LD))[:, None] * LD(U)
    out = []
    for v, A in ((d, dA), (l, lA)):
        pb = (fac * A).sum()
        out.append((v.sum(), pb + LD(v.size) * LD(U) * (np.abs(v).sum() + pb)))
    return (out[0][0], out[1][0]), (out[0][1], out[1][1])


FACES = {2: ((0, 1), (1, 2), (2, 0)), 3: ((0, 1, 2), (1, 0, 3), (0, 2, 3), (2, 1, 3))}      # deal.II local faces, as host/frontend.cpp lists them


class FaceTablesLike:
    """the fields Nsx.set_force_faces reads"""


def face_tables(dim, n_qf, seed=5):
    """a synthetic face rule in the layout nsx_set_force_faces reads ([local face][point] rows): n_qf seeded points strictly inside every
    local face (n_qf = 1: its centroid), positive weights summing to 1 -- arithmetic, not quadrature exactness, is what it serves"""
    rng = np.random.default_rng(seed + n_qf)
    bary = rng.dirichlet(np.full(dim, 2.0), size=n_qf) if n_qf > 1 else np.full((1, dim), 1.0 / dim)
    verts = np.concatenate([np.zeros((1, dim)), np.eye(dim)], axis=0)
    pts = np.concatenate([bary @ verts[list(f)] for f in FACES[dim]], axis=0)
    w = rng.uniform(0.5, 1.5, size=n_qf)
    t = tables_from_points(dim, pts, np.tile(w / w.sum(), dim + 1))
    ft = FaceTablesLike()
    ft.n_qf, ft.N2, ft.dN2, ft.N1, ft.weights = n_qf, t.N2, t.dN2, t.N1, t.weights
    return ft


def all_faces(topo, geo, ftab, cells):
    """every local face 0..dim of the listed cells as (cells, local faces, skipped); in 3D without the faces whose normal has
    nx^2 + ny^2 < 1e-6: the tangential formula divides by that"""
    dim = topo.dim
    cells = np.asarray(cells, dtype=np.int64)
    cells, lf = np.repeat(cells, dim + 1), np.tile(np.arange(dim + 1), len(cells))
    if dim == 2:
        return cells.astype(np.int32), lf.astype(np.int32), 0
    t2 = forces_points(topo, geo, ftab, np.zeros(topo.n_u + topo.n_p), cells, lf, 1.0)[2]
    keep = np.asarray(t2 >= 1e-6)
    return cells[keep].astype(np.int32), lf[keep].astype(np.int32), int((~keep).sum())


# ------------------------------------------------------------------------------------------------------------------ float64 restatement
def restate(dofs, tables, nu, deltat, x, flags=0, first=True, order="kernel", mutant=None, topo=None, coords=None, static=None):
    """The float64 restatement of the same formulas: dict of float64 arrays on the padded graphs (mass, stiff, conv, F, G, B, pmass,
    rhs).  order: kernel / reversed / pairwise summation everywhere.  mutant: one of MUTANTS that acts on the assembly
    (lost_half, signed_det, swapped_ji, weight, gather_tail, conv_scale).  static: an earlier result of the same mesh, tables, order and
    mutant whose state-independent parts are taken over."""
    topo = topo or Topology(dofs)
    dim = topo.dim
    t = cast_tables(tables, np.float64)
    if mutant == "weight":
        w = t.weights.copy()
        w[len(w) // 2] *= 1.0 + 1e-12
        t = TablesLike(dim, None, w, t.N2, t.dN2, t.N1)
    g = geometry(dofs.cell_coords if coords is None else coords, np.float64)
    Ji = np.ascontiguousarray(np.transpose(g.Ji, (0, 2, 1))) if mutant == "swapped_ji" else g.Ji
    adet = g.det if mutant == "signed_det" else g.adet
    temam = bool(flags & TEMAM)
    cs = 2 if (first and flags & DOUBLE_CONVECTION and mutant != "conv_scale") else 1
    u = cell_values(topo, np.asarray(x, dtype=np.float64))
    conv = convection_block(Ji, adet, t, u, temam, cs, order, half=1.0 if mutant == "lost_half" else 0.5)
    drop = mutant == "gather_tail"
    ga = lambda b, el: topo.to_padded(b, gather(topo, b, el, order, drop)[0])
    if static is not None:
        out = {k: static[k] for k in ("mass", "stiff", "G", "B", "pmass")}
    else:
        mass, stiff, D, pm = static_blocks(Ji, adet, t, np.float64(nu), np.float64(deltat), order)
        out = {"mass": ga(0, mass), "stiff": ga(0, stiff), "G": -ga(1, D), "B": ga(2, np.transpose(D, (0, 2, 1, 3))), "pmass": ga(3, pm)}
    out["conv"] = ga(0, conv)
    out["F"] = (out["mass"] + out["stiff"]) + out["conv"]
    rp, ci = topo.padded[0]
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    xs = np.asarray(x, dtype=np.float64)
    rhs = np.zeros(len(xs))
    same = (rows % dim) == (ci % dim)
    terms = (out["mass"] * xs[ci])[same]
    r = rows[same]
    if order == "reversed":
        terms, r = terms[::-1], r[::-1]
    np.add.at(rhs, r, terms)
    out["rhs"] = rhs
    return out


def check_state(ref_state, got, names=None):
    """got: dict name -> float64 values; -> (messages, {name: ratio})"""
    msgs, ratios = [], {}
    for k in names or got:
        m, ratios[k] = ref_state[k].check(got[k], k)
        msgs += m
    return msgs, ratios


# ------------------------------------------------------------------------------------------------------------------ meshes and states
NU, DELTAT = 1.37e-3, 3.3e-3          # not round numbers
MESHES = {"b2a": ("box", 2, dict(n=[1, 1])), "b2b": ("box", 2, dict(n=[4, 8])), "b2c": ("box", 2, dict(n=[3, 11], hi=[1.0, 1e-4])),
          "c2": ("cylinder", 2, dict(level=2)), "b3a": ("box", 3, dict(n=[1, 1, 1])), "b3b": ("box", 3, dict(n=[2, 2, 3], hi=[1.0, 1e-3, 1e3])),
          "b3c": ("box", 3, dict(n=[1, 1, 11])), "c3": ("cylinder", 3, dict(level=1)), "s2": ("sheared", 2, {}), "s3": ("sheared", 3, {})}
N_CELLS = {"b2a": 2, "b2b": 64, "b2c": 66, "c2": 632, "b3a": 6, "b3b": 72, "b3c": 66, "c3": 2832, "s2": 3, "s3": 3}
# three sheared cells in a row, every one a sliver whose determinant is a difference of products a thousand times larger
SHEARED = {2: ([(0, 0), (1, 1), (1.001, 1.002), (2.001, 2.002), (2.002, 2.004)], [(0, 1, 2), (1, 3, 2), (2, 3, 4)]),
           3: ([(0, 0, 0), (1, 1, 1), (1.03, 1.01, 1.0), (1.0, 1.02, 1.04), (2.0, 2.01, 2.03), (2.05, 2.0, 2.02)],
               [(0, 1, 2, 3), (1, 2, 3, 4), (2, 3, 4, 5)])}


def write_msh(path, verts, cells):
    dim = len(verts[0])
    with open(path, "w") as f:
        f.write("$MeshFormat\n2.2 0 8\n$EndMeshFormat\n$Nodes\n%d\n" % len(verts))
        for i, v in enumerate(verts):
            f.write("%d %.17g %.17g %.17g\n" % ((i + 1,) + tuple(list(v) + [0.0] * (3 - dim))))
        f.write("$EndNodes\n$Elements\n%d\n" % len(cells))
        for i, c in enumerate(cells):
            f.write("%d %d 2 10 1 %s\n" % (i + 1, 4 if dim == 3 else 2, " ".join(str(k + 1) for k in c)))
        f.write("$EndElements\n")


def build_mesh(name, n_sub=1):
    """(mesh, dofs) of MESHES[name]"""
    import os
    import tempfile
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh
    kind, dim, kw = MESHES[name]
    if kind == "box":
        mesh = Mesh.box(dim, kw["n"], hi=kw.get("hi"))
    elif kind == "cylinder":
        mesh = Mesh.cylinder(dim, kw["level"])
    else:
        with tempfile.TemporaryDirectory() as d:
            write_msh(os.path.join(d, "cells.msh"), *SHEARED[dim])
            mesh = Mesh.read_msh(os.path.join(d, "cells.msh"))
    assert mesh.cells.shape[0] == N_CELLS[name], (name, mesh.cells.shape)
    if n_sub > 1:
        mesh.partition(1, n_sub)
    return mesh, DoFs(mesh)


def velocity(name, dofs, seed=0):
    """smooth_velocity on the cylinders; elsewhere a seeded vector whose components spread over six decades"""
    import types
    if MESHES[name][0] == "cylinder":
        from conftest import Problem
        return Problem.smooth_velocity(types.SimpleNamespace(dofs=dofs, kind="cylinder", dim=dofs.dim), seed=1234 + seed, amp=1.0 - 0.1 * seed)
    rng = np.random.default_rng(77 + seed)
    return rng.standard_normal(dofs.n_dofs) * 10.0 ** rng.uniform(-3, 3, dofs.n_dofs)


def dirichlet_map(name, dofs, time=DELTAT):
    """the existing boundary helpers on the cylinders, the face x = 0 (boundary id 0) elsewhere; sorted by dof, whole nodes"""
    if MESHES[name][0] == "cylinder":
        from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
        return cylinder_boundary_values(dofs, InletVelocity(dofs.dim, 2), time)
    bd = np.sort(dofs.boundary_dofs(0)).astype(np.int32)
    return bd, np.linspace(0.5, 1.5, len(bd)) * (1.0 + time)
