"""Extended-precision restatement of the sparse products of csrc/nsx_sparse.hip (the ops of nsx_sparse_product, include/nsx.h), the
entry-by-entry bound the device results are held to, and the chunk table of the LDS-staged kernel (spmv_chunks / build_blocked of
csrc/nsx_setup.hip) restated on the host.  Shared by tests/test_sparse_reference.py (CPU) and tests/test_gpu_sparse.py.

Reference.  Every op is a plain loop over the rows of CSR data in np.longdouble (64-bit significand on x86): for output entry i it
yields the value y_i, the number n_i of terms a_ij x_j of its sum and A_i = sum_j |a_ij x_j| (+ |aux_i| for the fused ops).

Bound (derived, not measured).  Whatever the order of the summation and wherever an FMA is used, a float64 sum of n terms
satisfies |fl(sum) - sum| <= gamma_n A with gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability, section 3.1 / 4.2: the
products count as one rounding each, an FMA only removes one).  The fused ops subtract or add aux to the FINISHED row sum: one more
rounding, u |y_i| <= u (A_i + |aux_i|) (1 + gamma_n).  With n u < 1e-13 on every matrix here, gamma_n A + u (...) < (n + 2) u A, so

        |y_dev_i - y_ref_i| <= (n_i + 2) * 2^-53 * A_i          for every entry i,

and an entry with A_i = 0 (an empty row, x = 0, an entry the op does not produce) must be exactly 0.0.  The saddle product adds the
block(0,1) row to the F row: n_i counts both rows' entries, A_i both rows' terms; the bound covers the plain kernel (one sum over
both) and the staged path (F, then += G: two sums and one addition) alike.  The reference's own error is (n_i + 1) 2^-64 A_i, 2^-11 of
the bound: it is not added.
The float stream (NSX_INNER_FP32) computes in double on values rounded to float: its reference is the same loop on
F.astype(np.float32).astype(np.longdouble), under the same bound."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
# the ops in the order of NSX_PROD_* (include/nsx.h)
OPS = ("F", "F_INNER", "F_RESID", "MASS", "B", "B_MINUS_R", "R_MINUS_B", "G", "G_ACC", "S", "SADDLE")
NEEDS_AUX = {"F_RESID", "B_MINUS_R", "R_MINUS_B", "G_ACC"}
U_OPS = {"F", "F_INNER", "F_RESID", "MASS", "G", "G_ACC"}     # ops whose result lives in the velocity part
P_OPS = {"B", "B_MINUS_R", "R_MINUS_B", "S"}


class Operators:
    """the matrices of one handle in the caller's numbering.  F, mass: values on the SCALAR P2 graph (rp, ci) -- one entry serves the dim
    interleaved components, as on the device; B (n_p x n_u), G (n_u x n_p), S (n_p x n_p): plain CSR over dofs."""

    def __init__(self, dim, n_u, n_p, f_graph, F, mass, B, G, S=None):
        self.dim, self.n_u, self.n_p, self.n2 = dim, n_u, n_p, n_u // dim
        self.rp, self.ci = (np.asarray(a, dtype=np.int64) for a in f_graph)
        self.F, self.mass = np.asarray(F, dtype=np.float64), np.asarray(mass, dtype=np.float64)
        self.B, self.G, self.S = B, G, S        # (rp, ci, values) each
        assert len(self.rp) == self.n2 + 1 and len(self.F) == len(self.ci) == len(self.mass)

    def with_float_F(self):
        """the operators the float stream reads: F rounded to float (everything else is read as double)"""
        o = Operators.__new__(Operators)
        o.__dict__.update(self.__dict__)
        o.F = self.F.astype(np.float32).astype(np.float64)
        return o


def scalar_selection(dofs):
    """(mask over the entries of the padded block(0,0) graph that carry the scalar operator, its scalar graph): the same-component
    entries of the rows of component 0"""
    rp, ci = dofs.reference_sparsity(0)
    dim = dofs.dim
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    sel = (rows % dim == 0) & (np.asarray(ci) % dim == 0)
    counts = np.bincount(rows[sel] // dim, minlength=dofs.n_u // dim)
    return sel, (np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), (np.asarray(ci)[sel] // dim).astype(np.int32))


def operators_from(dofs, export, schur=None):
    """Operators from export(which, block) -> values on dofs.reference_sparsity(block) (Nsx.export_block / Oracle.matrix) and an
    optional scipy CSR Schur matrix"""
    sel, graph = scalar_selection(dofs)
    gG, gB = dofs.reference_sparsity(1), dofs.reference_sparsity(2)
    S = None if schur is None else (np.asarray(schur.indptr), np.asarray(schur.indices), np.asarray(schur.data, dtype=np.float64))
    return Operators(dofs.dim, dofs.n_u, dofs.n_p, graph, np.array(export(0, 0))[sel], np.array(export(1, 0))[sel],
                     (np.asarray(gB[0]), np.asarray(gB[1]), np.array(export(0, 2))), (np.asarray(gG[0]), np.asarray(gG[1]), np.array(export(0, 1))), S)


def _row_loop(rp, t):
    """for every row i: (sum, sum of absolute values) of the terms t[rp[i]:rp[i+1]] (t: [nnz] or [nnz][k]) in long double"""
    n = len(rp) - 1
    y, A = np.zeros((n,) + t.shape[1:], dtype=LD), np.zeros((n,) + t.shape[1:], dtype=LD)
    for i in range(n):
        s = t[rp[i]:rp[i + 1]]
        if len(s):
            y[i], A[i] = s.sum(axis=0), np.abs(s).sum(axis=0)
    return y, A


class Result:
    """y, n, A of one op over the whole block vector (entries the op does not produce: 0, 0, 0)"""

    def __init__(self, n_u, n_p):
        self.n_u = n_u
        self.y, self.A, self.n = np.zeros(n_u + n_p, dtype=LD), np.zeros(n_u + n_p, dtype=LD), np.zeros(n_u + n_p, dtype=np.int64)

    def bound(self):
        return (self.n + 2).astype(LD) * LD(U) * self.A

    def add(self, lo, y, A, n):
        hi = lo + len(y)
        self.y[lo:hi] += y
        self.A[lo:hi] += A
        self.n[lo:hi] += n


def _scalar(o, vals, x):
    X = np.asarray(x[:o.n_u], dtype=LD).reshape(o.n2, o.dim)
    y, A = _row_loop(o.rp, vals.astype(LD)[:, None] * X[o.ci])
    return y.reshape(-1), A.reshape(-1), np.repeat(np.diff(o.rp), o.dim)


def _csr(m, x):
    rp, ci, v = m
    y, A = _row_loop(rp, v.astype(LD) * np.asarray(x, dtype=LD)[ci])
    return y, A, np.diff(rp)


def reference(o, op, x, aux=None):
    """Result of op (a name of OPS) on the block vector x (and aux)"""
    assert op in OPS and (aux is not None or op not in NEEDS_AUX)
    r = Result(o.n_u, o.n_p)
    xu, xp = x[:o.n_u], x[o.n_u:]
    if op in ("F", "F_INNER", "F_RESID", "MASS", "SADDLE"):
        r.add(0, *_scalar(o, o.mass if op == "MASS" else o.F, x))
    if op in ("G", "G_ACC", "SADDLE"):
        r.add(0, *_csr(o.G, xp))
    if op in ("B", "B_MINUS_R", "R_MINUS_B", "SADDLE"):
        r.add(o.n_u, *_csr(o.B, xu))
    if op == "S":
        r.add(o.n_u, *_csr(o.S, xp))
    if op in NEEDS_AUX:
        a = np.asarray(aux, dtype=LD)
        lo, hi = (0, o.n_u) if op in U_OPS else (o.n_u, o.n_u + o.n_p)
        sign = -1 if op in ("F_RESID", "R_MINUS_B") else 1      # F_RESID, R_MINUS_B: aux - sum; B_MINUS_R: sum - aux; G_ACC: aux + sum
        r.y[lo:hi] = sign * r.y[lo:hi] + (a[lo:hi] if op != "B_MINUS_R" else -a[lo:hi])
        r.A[lo:hi] += np.abs(a[lo:hi])
    return r


def compare(ref, y):
    """(messages of the entries outside the bound, largest error / bound over the entries with a bound > 0)"""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == ref.y.shape
    err, bound = np.abs(y.astype(LD) - ref.y), ref.bound()
    bad = np.nonzero(~(err <= bound))[0]            # NaN fails
    msgs = ["entry %d (%s part): %.17g, reference %.17g, error %.3e > bound %.3e (n = %d)" %
            (i, "velocity" if i < ref.n_u else "pressure", y[i], float(ref.y[i]), float(err[i]), float(bound[i]), ref.n[i]) for i in bad[:5]]
    if len(bad) > 5:
        msgs.append("... and %d more entries" % (len(bad) - 5))
    pos = bound > 0
    ratio = float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0
    return msgs, ratio


def column(o, op, j):
    """column j (a dof of the block vector) of the matrix of a product op WITHOUT aux, as float64 over the block vector: what the op must
    return bit for bit for the unit vector e_j (products with 1 and sums with 0 are exact)"""
    out = np.zeros(o.n_u + o.n_p)

    def csr_col(m, jj, lo):
        rp, ci, v = m
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        hit = np.asarray(ci) == jj
        assert len(np.unique(rows[hit])) == hit.sum()           # one entry per row and column
        out[lo + rows[hit]] += v[hit]

    if op in ("F", "F_INNER", "MASS", "SADDLE") and j < o.n_u:
        node, c = divmod(j, o.dim)
        rows = np.repeat(np.arange(o.n2), np.diff(o.rp))
        hit = o.ci == node
        out[rows[hit] * o.dim + c] += (o.mass if op == "MASS" else o.F)[hit]
    if op in ("G", "SADDLE") and j >= o.n_u:
        csr_col(o.G, j - o.n_u, 0)
    if op in ("B", "SADDLE") and j < o.n_u:
        csr_col(o.B, j, o.n_u)
    if op == "S" and j >= o.n_u:
        csr_col(o.S, j - o.n_u, o.n_u)
    return out


# ------------------------------------------------------------------------------------------------ float64 restatements (CPU suite)
def _sum64(t, order):
    """float64 sum of the terms t of one row in one of three orders: "forward", "reversed", or "lanes16" -- lane l of 16 adds the
    terms l, l + 16, ... in turn, then the butterfly of lane_group_sum<16> (csrc/nsx_internal.hpp): xor 1, xor 2, mirror in 8, mirror in 16"""
    if order == "lanes16":
        v = np.zeros(16)
        for k, tk in enumerate(t):
            v[k % 16] += tk
        lane = np.arange(16)
        for perm in (lane ^ 1, lane ^ 2, (lane & 8) | (7 - (lane & 7)), 15 - lane):
            v = v + v[perm]
        return v[0]
    acc = 0.0
    for tk in (t if order == "forward" else t[::-1]):
        acc += tk
    return acc


def product64(o, op, x, aux=None, order="forward"):
    """op in float64 arithmetic, every row summed in the given order; the fused epilogues act on the finished sum, as on the device"""
    out = np.zeros(o.n_u + o.n_p)
    xu, xp = np.asarray(x[:o.n_u], dtype=np.float64), np.asarray(x[o.n_u:], dtype=np.float64)

    def csr(m, v, lo):
        rp, ci, a = m
        for i in range(len(rp) - 1):
            out[lo + i] += _sum64(a[rp[i]:rp[i + 1]] * v[ci[rp[i]:rp[i + 1]]], order)

    if op in ("F", "F_INNER", "F_RESID", "MASS", "SADDLE"):
        vals, X = (o.mass if op == "MASS" else o.F), xu.reshape(o.n2, o.dim)
        for i in range(o.n2):
            sl = slice(o.rp[i], o.rp[i + 1])
            for c in range(o.dim):
                out[i * o.dim + c] = _sum64(vals[sl] * X[o.ci[sl], c], order)
    if op in ("G", "G_ACC", "SADDLE"):
        csr(o.G, xp, 0)
    if op in ("B", "B_MINUS_R", "R_MINUS_B", "SADDLE"):
        csr(o.B, xu, o.n_u)
    if op == "S":
        csr(o.S, xp, o.n_u)
    if op in NEEDS_AUX:
        a = np.asarray(aux, dtype=np.float64)
        sl = slice(0, o.n_u) if op in U_OPS else slice(o.n_u, o.n_u + o.n_p)
        out[sl] = out[sl] - a[sl] if op == "B_MINUS_R" else a[sl] + out[sl] if op == "G_ACC" else a[sl] - out[sl]
    return out


def vectors(n, seed=20250101):
    """the seeded standard-normal x and aux of the suites"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n)


# ------------------------------------------------------------------------------------------------ the chunk table, restated
def spmv_chunks(n, rank_ptr, target=130):
    """chunk bounds of the LDS-staged SpMV for n rows and a rank table in rows (None / one rank: no table), as spmv_chunks of
    csrc/nsx_setup.hip cuts them; target = NSX_SPMV_R clamped to 16..448, default 130"""
    target = max(16, min(448, int(target)))
    rk = [0, n] if rank_ptr is None else [int(v) for v in rank_ptr]
    bounds = [0]
    many = len(rk) > 2
    by_rank = many and n / (len(rk) - 1) <= target
    split_ranks = not by_rank and many and n / (len(rk) - 1) <= 4.0 * target
    if by_rank:
        start = 0
        for r in range(1, len(rk)):
            if rk[r] - start > target and rk[r - 1] > start:      # close the chunk in front of a rank that would take it past the target
                bounds.append(rk[r - 1])
                start = rk[r - 1]
        bounds.append(n)
    elif split_ranks:
        for r in range(len(rk) - 1):
            rows = rk[r + 1] - rk[r]
            if rows <= 0:
                continue
            parts = (rows + target - 1) // target
            bounds += [rk[r] + rows * q // parts for q in range(1, parts + 1)]
        if bounds[-1] != n:
            bounds.append(n)
    else:
        bounds += list(range(128, n, 128)) + [n]
    out = [0]
    for b in bounds[1:]:
        while b - out[-1] > 448:                                   # the kernel's row-pointer buffer: oversized chunks are cut at 224 rows
            out.append(out[-1] + 224)
        if b > out[-1]:
            out.append(b)
    return np.array(out, dtype=np.int64)


def chunk_stats(rp, ci, bounds):
    """(chunks, rows of the largest chunk, staged columns of the chunk that stages most, staged column list per chunk) as build_blocked
    counts them"""
    rp, ci = np.asarray(rp), np.asarray(ci)
    cols = [np.unique(ci[rp[a]:rp[b]]) for a, b in zip(bounds[:-1], bounds[1:])]
    return len(bounds) - 1, int(np.max(np.diff(bounds))), max(len(c) for c in cols), cols


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def block_ptr(n, rows):
    return np.array(list(range(0, n, rows)) + [n], dtype=np.int32)


def crafted_ranks(n, small, separators, fill=130):
    """rank table (in rows) whose chunks at NSX_SPMV_R = 448 include one of exactly s rows for every s of `small`: each small rank is
    followed by a separator rank that would take its chunk past 448 rows, which closes the chunk in front of it -- and the next small
    rank closes the separator's.  The rest: ranks of `fill` rows, an empty rank, and the remainder."""
    assert len(small) == len(separators) and all(s + q > 448 for s, q in zip(small, separators)) and all(q + s > 448 for q, s in zip(separators, small[1:]))
    sizes = [v for pair in zip(small, separators) for v in pair]
    rest = n - sum(sizes)
    assert rest > 0
    tail = [fill] * (rest // fill)
    tail.insert(min(1, len(tail)), 0)
    if rest % fill:
        tail.append(rest % fill)
    return ptr_of(sizes + tail)


# the tables of tests/test_gpu_sparse.py (A: 4806 rows, B: 1364 rows) and the chunk sizes they must yield at NSX_SPMV_R = 448
CRAFTED = {4806: dict(small=[1, 15, 16, 17, 31, 32, 33], separators=[448, 447, 449, 440, 430, 420, 416]),
           1364: dict(small=[1, 17, 33], separators=[448, 440, 420])}
CRAFTED_SIZES = {4806: [1, 448, 15, 447, 16, 224, 225, 17, 440, 31, 430, 32, 420, 33, 416, 390, 390, 390, 441],
                 1364: [1, 448, 17, 440, 33, 425]}
