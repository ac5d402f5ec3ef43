"""Extended-precision restatement of the per-step preconditioner set-up of prec_initialize (csrc/nsx_solve.hip, csrc/nsx_sparse.hip):
the diagonal D (k_extract_diag), its reciprocals (k_reciprocal), the lumped mass (k_abs_rowsum + k_reciprocal), the weights of the Schur
product w = -V * mask and the product S = B diag(w) B^T itself (k_schur<2|3>), with the agreement each is held to.  Shared by
tests/test_prec_setup_reference.py (CPU, the oracle's matrices) and tests/test_gpu_prec_setup.py (the device's own matrices).

Input (class Setup).  The scalar F and mass values on the scalar P2 graph (sparse_reference.operators_from / scalar_selection), block(1,0)
as CSR over dofs, the constrained dofs, dim; and the preconditioner type.

Quantities and what is asserted of each.
  D          the diagonal entry of mass (Yosida) or of F (SIMPLE, aSIMPLE, aYosida), replicated on the dim components: a copy, so equal bit
             for bit to the exported matrix entry.
  D_inv, neg_D_inv   np.float64(+-1.0) / D: IEEE double division is correctly rounded and the build has no fast-math, so equal bit for bit.
  lump_M     -1 / sum_j |M_ij| over the n_i entries of the scalar row.  The terms |M_ij| carry no rounding, a float64 sum of n_i of them in
             any order has a relative error of at most gamma_{n_i - 1} (all terms are of one sign: A = the sum itself), the division adds one
             rounding: (1 + gamma_{n_i-1})(1 + u) - 1 < (n_i + 2) u for n_i u < 1e-13, so
                     |dev - ref| <= (n_i + 2) * 2^-53 * |ref|.
  w          -V * mask with V = neg_D_inv (aYosida: lump_M) and mask in {0, 1}: products with 0, 1 and -1 are exact, so w is asserted bit
             for bit from the DEVICE's own V and mask.
  S_ij       sum over the dofs k = (node, c) that row i and row j of B share of B[i,k] * w[k] * B[j,k], with the DEVICE's exported w (the
             weights have their own assertion; S is judged for what the product kernel does with them).

Bound on S (derived, not measured).  The kernel stages fl(B[i,k] w[k]) and multiplies by B[j,k]: every term carries two roundings,
|fl(fl(B w) B) - B w B| <= (2 u + u^2) |B w B| (an FMA for the second product removes one of them).  A float64 sum of n terms in any
order, with or without FMA, adds gamma_{n-1} times the sum of the absolute values of the (rounded) terms (Higham, Accuracy and Stability,
section 4.2).  Together: |dev - ref| <= ((1 + 2u + u^2)(1 + gamma_{n-1}) - 1) A < (n + 3) u A for n u < 1e-13 (n <= 228 here), A_ij =
sum |B w B| and n_ij the number of scalar terms (common dofs, structural).  So

        |S_dev_ij - S_ref_ij| <= (n_ij + 3) * 2^-53 * A_ij          for every stored entry,

and an entry with A_ij = 0 -- every common column constrained, so every term is a product with w = 0 -- must be exactly 0.0.  The
reference's own error (three-factor products and n additions in long double: (n + 2) 2^-64 A) is 2^-11 of the bound and is not added.

schur64 / weights64 restate the computation in float64; MUTANTS are wrong versions of them, each of which must leave its bound or the
exact-zero condition (tests/test_prec_setup_reference.py):
  no_abs         lump_M without the absolute value (the mass matrix has negative entries)
  mask_dropped   weights without the Dirichlet mask
  last_common    the last common column (node) of every pair of rows left out: the merge cursor stopping one early
  one_component  component dim - 1 left out
  tail_row       entries beyond the 64th of a Schur row left at their previous value: the 64-stride loop without its second trip
  ghost_weight   weights of the columns row i's rank does not own taken as 0: the halo exchange of w missing"""
import numpy as np

import sparse_reference as SR

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended-precision long double (x87: eps 1.08e-19)"
U = 2.0 ** -53
YOSIDA, SIMPLE, AYOSIDA, ASIMPLE = 0, 1, 2, 3           # NSX_PREC_* (include/nsx.h)
TYPES = {"yosida": YOSIDA, "simple": SIMPLE, "ayosida": AYOSIDA, "asimple": ASIMPLE}
MUTANTS = ("no_abs", "mask_dropped", "last_common", "one_component", "tail_row", "ghost_weight")


class Setup:
    """the inputs of one set-up in the caller's numbering, and the term structure of the Schur product (a function of the graph of
    block(1,0) alone: built once, shared by every set of values on that graph through `like`)"""

    def __init__(self, dim, f_graph, F, mass, B, constrained, like=None):
        self.dim = dim
        self.rp, self.ci = (np.asarray(a, dtype=np.int64) for a in f_graph)
        self.n2 = len(self.rp) - 1
        self.n_u = self.n2 * dim
        self.F, self.mass = np.asarray(F, dtype=np.float64), np.asarray(mass, dtype=np.float64)
        self.Brp, self.Bci, self.Bv = np.asarray(B[0], dtype=np.int64), np.asarray(B[1], dtype=np.int64), np.asarray(B[2], dtype=np.float64)
        self.n_p = len(self.Brp) - 1
        self.constrained = np.asarray(constrained, dtype=np.int64)
        assert len(self.F) == len(self.mass) == len(self.ci) and len(self.Bv) == len(self.Bci)
        rows = np.repeat(np.arange(self.n2), np.diff(self.rp))
        self.diag = np.nonzero(self.ci == rows)[0]
        assert len(self.diag) == self.n2                 # one diagonal entry per scalar row
        if like is not None:
            assert np.array_equal(like.Brp, self.Brp) and np.array_equal(like.Bci, self.Bci)
            self.terms = like.terms
        else:
            self.terms = _terms(self.Brp, self.Bci, self.n_p, self.n_u, dim)

    def mask(self):
        m = np.ones(self.n_u)
        m[self.constrained] = 0.0
        return m


def setup_from(dofs, export, constrained, like=None):
    """Setup from export(which, block) -> values on dofs.reference_sparsity(block) (Nsx.export_block / Oracle.matrix)"""
    o = SR.operators_from(dofs, export)
    return Setup(dofs.dim, (o.rp, o.ci), o.F, o.mass, o.B, constrained, like)


class Terms:
    """every scalar term of S = B diag(w) B^T, sorted by (row i, column j, dof k): e = entry of S it belongs to, pi / pj = positions of
    B[i,k] / B[j,k] in the values of B, k = the common dof; (rp, ci) = the graph of S, seg = first term of every entry"""


def _terms(Brp, Bci, n_p, n_u, dim):
    rows = np.repeat(np.arange(n_p), np.diff(Brp))
    order = np.lexsort((rows, Bci))                      # the entries of B by column, rows ascending inside a column
    counts = np.bincount(Bci, minlength=n_u)
    starts = np.concatenate([[0], np.cumsum(counts)])
    PI, PJ, K = [], [], []
    for c in np.unique(counts):
        if c == 0:
            continue
        cols = np.nonzero(counts == c)[0]
        pos = order[starts[cols][:, None] + np.arange(c)[None, :]]          # [columns with c entries][c]: positions in B
        shape = (len(cols), c, c)
        PI.append(np.broadcast_to(pos[:, :, None], shape).ravel())
        PJ.append(np.broadcast_to(pos[:, None, :], shape).ravel())
        K.append(np.broadcast_to(cols[:, None, None], shape).ravel())
    t = Terms()
    pi, pj, k = np.concatenate(PI), np.concatenate(PJ), np.concatenate(K)
    key = rows[pi] * n_p + rows[pj]
    srt = np.lexsort((k, key))
    t.pi, t.pj, t.k, key = pi[srt], pj[srt], k[srt], key[srt]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    t.seg = np.nonzero(first)[0]
    t.e = np.cumsum(first) - 1
    ekey = key[t.seg]
    t.ci = (ekey % n_p).astype(np.int32)
    t.rp = np.concatenate([[0], np.cumsum(np.bincount(ekey // n_p, minlength=n_p))]).astype(np.int32)
    t.n = np.diff(np.concatenate([t.seg, [len(key)]]))
    t.row = (ekey // n_p).astype(np.int64)
    t.n_p, t.dim = n_p, dim
    return t


# ------------------------------------------------------------------------------------------------------------------ vectors
def diagonal(s, ptype):
    """D in float64: a copy of the matrix entry"""
    assert ptype in TYPES.values()
    return np.repeat((s.mass if ptype == YOSIDA else s.F)[s.diag], s.dim)


class Lump:
    """lump_M in long double, the row lengths n_i and the bound, per velocity dof"""

    def __init__(self, s):
        a = np.add.reduceat(np.abs(s.mass).astype(LD), s.rp[:-1])
        assert np.all(np.diff(s.rp) > 0) and np.all(a > 0)
        self.y = np.repeat(LD(-1) / a, s.dim)
        self.n = np.repeat(np.diff(s.rp), s.dim)

    def bound(self):
        return (self.n + 2).astype(LD) * LD(U) * np.abs(self.y)


def compare_lump(ref, v):
    """(messages of the entries of lump_M outside the bound, largest error / bound)"""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape == ref.y.shape
    err, bound = np.abs(v.astype(LD) - ref.y), ref.bound()
    bad = np.nonzero(~(err <= bound))[0]
    msgs = ["lump_M[%d]: %.17g, reference %.17g, error %.3e > bound %.3e (n = %d)" % (i, v[i], float(ref.y[i]), float(err[i]), float(bound[i]), ref.n[i])
            for i in bad[:5]]
    if len(bad) > 5:
        msgs.append("... and %d more entries" % (len(bad) - 5))
    return msgs, float(np.max(err / bound))


def _forward_rowsum(rp, v):
    """float64 sum of every row of v, one term after the other in the row's order (k_abs_rowsum, and the oracle)"""
    length, acc = np.diff(rp), np.zeros(len(rp) - 1)
    for t in range(int(length.max())):
        sel = length > t
        acc[sel] += v[rp[:-1][sel] + t]
    return acc


def weights64(s, ptype, mutant=None):
    """the vectors of the set-up as float64 arithmetic gives them: D, D_inv, neg_D_inv, lump_M (None unless aYosida), mask, w"""
    assert mutant is None or mutant in MUTANTS
    D = diagonal(s, ptype)
    out = {"D": D, "D_inv": np.float64(1.0) / D, "neg_D_inv": np.float64(-1.0) / D, "lump_M": None, "mask": s.mask()}
    V = out["neg_D_inv"]
    if ptype == AYOSIDA:
        m = s.mass if mutant == "no_abs" else np.abs(s.mass)
        with np.errstate(divide="ignore"):               # no_abs: a row of the mass matrix may sum to 0
            V = out["lump_M"] = np.repeat(np.float64(-1.0) / _forward_rowsum(s.rp, m), s.dim)
    with np.errstate(invalid="ignore"):
        out["w"] = -V * (1.0 if mutant == "mask_dropped" else out["mask"])
    return out


def weights_of(V, mask):
    """w from the device's own V and mask: exact products"""
    return -(np.asarray(V, dtype=np.float64) * np.asarray(mask, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------------ the product
class Schur:
    """S in long double on the graph (rp, ci): y, the sums A of the absolute terms, the term counts n"""

    def __init__(self, s, w):
        t = s.terms
        w = np.asarray(w, dtype=np.float64)
        assert w.shape == (s.n_u,)
        term = s.Bv[t.pi].astype(LD) * w[t.k].astype(LD) * s.Bv[t.pj].astype(LD)
        self.y, self.A, self.n = np.add.reduceat(term, t.seg), np.add.reduceat(np.abs(term), t.seg), t.n
        self.rp, self.ci, self.row = t.rp, t.ci, t.row

    def bound(self):
        return (self.n + 3).astype(LD) * LD(U) * self.A


def compare_schur(ref, values, limit=5):
    """(messages of the entries outside the bound or not exactly 0 where A = 0, largest error / bound over the entries with a bound > 0)"""
    v = np.asarray(values, dtype=np.float64)
    assert v.shape == ref.y.shape
    err, bound = np.abs(v.astype(LD) - ref.y), ref.bound()
    bad = np.nonzero(~(err <= bound))[0]             # NaN fails; where A = 0 the bound is 0: only 0.0 passes
    msgs = ["S[%d, %d]: %.17g, reference %.17g, error %.3e > bound %.3e (n = %d%s)" %
            (ref.row[e], ref.ci[e], v[e], float(ref.y[e]), float(err[e]), float(bound[e]), ref.n[e], ", every term masked: exactly 0 expected" if bound[e] == 0 else "")
            for e in bad[:limit]]
    if len(bad) > limit:
        msgs.append("... and %d more entries" % (len(bad) - limit))
    pos = bound > 0
    return msgs, (float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0)


def schur64(s, w, mutant=None, prev=None, u_ptr=None, p_ptr=None):
    """the values of S as float64 arithmetic gives them, term by term as the kernel forms them: fl(fl(B[i,k] w[k]) B[j,k]).  mutant: one
    of MUTANTS that acts on the product; prev: the values tail_row leaves in place (default 0); u_ptr / p_ptr: the rank tables (P2 nodes,
    pressure rows) of ghost_weight"""
    assert mutant is None or mutant in MUTANTS
    t = s.terms
    wk = np.asarray(w, dtype=np.float64)[t.k]
    if mutant == "ghost_weight":
        u_ptr, p_ptr = np.asarray(u_ptr), np.asarray(p_ptr)
        rank_i = np.searchsorted(p_ptr, t.row[t.e], side="right") - 1
        rank_k = np.searchsorted(u_ptr, t.k // s.dim, side="right") - 1
        wk = np.where(rank_i == rank_k, wk, 0.0)
    term = (s.Bv[t.pi] * wk) * s.Bv[t.pj]
    if mutant == "one_component":
        term = np.where(t.k % s.dim == s.dim - 1, 0.0, term)
    if mutant == "last_common":
        node = t.k // s.dim
        term = np.where(node == np.maximum.reduceat(node, t.seg)[t.e], 0.0, term)
    v = np.add.reduceat(term, t.seg)
    if mutant == "tail_row":
        place = np.arange(len(v)) - np.repeat(t.rp[:-1], np.diff(t.rp))
        v = np.where(place >= 64, np.zeros(len(v)) if prev is None else prev, v)
    return v
