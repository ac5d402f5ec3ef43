"""Extended-precision reference of the block-Jacobi ILU(0) (the factorisation, inversion and solve kernels of csrc/nsx_ilu.hip and
csrc/nsx_ilu_lanes.hpp), the yardstick they are measured with, and the comparisons the GPU tests call (tests/test_gpu_ilu.py; checked on
the CPU by tests/test_ilu_reference.py).  A plain helper module, no fixtures, NumPy only.

Storage is Ifpack's: strict lower = L, diagonal = 1/d, strict upper = U/d; every block restricted to its own rows and columns, entries
outside the blocks exactly 0.

* `factor(rp, ci, a, bptr, dtype, form)`: the sequential IKJ sweep per block, in np.longdouble (x87 extended, eps 1.08e-19: the
  reference) or in float64 in two groupings -- form "kernel": a_ik (U_kj / d_k) with the multiplier stored as a_ik (1 / d_k), what
  k_ilu_factor and its siblings compute; form "textbook": (a_ik / d_k) U_kj.  It also returns, per stored entry, the absolute-term sum
  s_ij = |a_ij| + sum_k |l_ik| |u_kj| carried through the storage transform (/ |d_j| for L, / |d_i| for U/d, / d_i^2 for 1/d): an entry's
  error is measured against s_ij, NOT against the entry (small entries are differences of large terms).
* `solve(rp, ci, lu, bptr, b, ncomp, dtype, mode, stream_float)`: x = U^-1 D^-1 L^-1 b per block for ncomp interleaved right-hand
  sides, by the sweeps (mode "sweep") or through explicit block inverses built column by column (mode "dense": k_ilu_invert* /
  k_ilu_apply_dense).  stream_float: the in-block off-diagonal entries pass through float as the lane-owner stream of a handle in FP32
  inner precision stores them (-L and -U/d rounded, 1/d kept double).  x is compared entry by entry, relative to max |x| of its block.
* `FactorReference` / `SolveReference`: the long-double result and err64, the larger deviation of the two float64 restatements from it
  on the same input.  A device result is accepted below K x (err64 + FLOOR), FLOOR = 4 eps; no asserted bound may reach
  HARD_LIMIT = 1e-11 (asserted in compare_factor / compare_solve).

The keyword switches skip_update / cross_block / unscaled_upper (factor) and skip_dinv / cross_block (solve) restate the operation
WRONGLY; tests/test_ilu_reference.py shows that the comparisons notice each of them."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended-precision long double (x87: eps 1.08e-19)"
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS
HARD_LIMIT = 1e-11
SEED = 2026

# Margins over the float64 restatements' own deviation: 10 x the largest ratio  error / (err64 + FLOOR)  measured on the MI355X over
# every case of tests/test_gpu_ilu.py (recorded as "ilu_unit"), rounded up.  Largest ratio per kernel:
#   factorisations  k_ilu_factor_lds 0.904 (2D Schur matrix, 96-row blocks)   k_ilu_factor_small 0.434
#                   k_ilu_factor 0.694 (3D Schur matrix as one block)   k_ilu_factor_level 0.509
#   solves          k_ilu_apply_dense behind k_ilu_invert_lds / k_ilu_invert 0.524 (identical for the two inversion kernels)
#                   k_ilu_solve_lanes NCOMP 1 / 2 / 3: 0.291 / 0.307 / 0.297 over E = 1..4 (PF 4 and 8 give identical numbers);
#                   k_ilu_solve_lanes_f32 NCOMP 2 / 3: 0.316 / 0.455, against the reference on the float-rounded entries
#                   k_ilu_solve<3, 8, true> 0.086   <3, 8, false> 0.088   k_ilu_solve_level NCOMP 1 / 2 / 3: 0.107 / 0.107 / 0.130
# -- every ratio is below 1: the kernels lose no more than the float64 restatements of the sequential sweep do, as they claim (the
# same operations in the same order; the solves differ from the sweeps only in the grouping of a row's sum).  No ratio needed an
# explanation, and no case failed.
K_FACTOR = 10.0      # 10 x 0.904, rounded up
K_SOLVE = 6.0        # 10 x 0.524, rounded up


def _blocks(bptr):
    bptr = np.asarray(bptr, dtype=np.int64)
    return [(int(a), int(b)) for a, b in zip(bptr[:-1], bptr[1:]) if b > a]


class Graph:
    """CSR graph + block table: per row the in-block range [lo, hi) of its (ascending) columns and the position of its diagonal"""

    def __init__(self, rp, ci, bptr):
        self.rp, self.ci, self.bptr = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(bptr, dtype=np.int64)
        self.n = n = len(self.rp) - 1
        assert self.bptr[0] == 0 and self.bptr[-1] == n and np.all(np.diff(self.bptr) >= 0)
        self.rows = np.repeat(np.arange(n), np.diff(self.rp))
        assert np.all(np.diff(self.ci)[np.diff(self.rows) == 0] > 0), "columns must ascend within a row"
        self.blk = np.searchsorted(self.bptr, np.arange(n), side="right") - 1
        r0, r1 = self.bptr[self.blk][self.rows], self.bptr[self.blk + 1][self.rows]
        self.inside = (self.ci >= r0) & (self.ci < r1)
        self.diag = np.flatnonzero(self.ci == self.rows)
        assert len(self.diag) == n
        self.lo = np.array([self.rp[i] + np.searchsorted(self.ci[self.rp[i]:self.rp[i + 1]], self.bptr[self.blk[i]]) for i in range(n)], dtype=np.int64)
        self.hi = np.array([self.rp[i] + np.searchsorted(self.ci[self.rp[i]:self.rp[i + 1]], self.bptr[self.blk[i] + 1]) for i in range(n)], dtype=np.int64)

    def cross_entry(self, a):
        """position of the strongest coupling (largest |a_ij / a_jj|) of a row to a row of an EARLIER block"""
        across = np.flatnonzero(self.ci < self.bptr[self.blk][self.rows])
        if not len(across):
            return None
        a = np.asarray(a, dtype=np.float64)
        return int(across[np.argmax(np.abs(a[across] / a[self.diag[self.ci[across]]]))])


def factor(rp, ci, a, bptr, dtype=LD, form="kernel", skip_update=None, cross_block=False, unscaled_upper=None, graph=None):
    """(lu, s): the block-Jacobi ILU(0) factors of a in Ifpack's storage, computed in `dtype`, and the absolute-term sums.
    WRONG variants: skip_update = row i: the FIRST pivot row's last in-block entry that has a partner in row i is left out of row i's
    update; cross_block: the strongest coupling to an earlier block keeps its multiplier a_ij / d_j; unscaled_upper = row whose upper
    triangle stays U instead of U / d."""
    g = graph or Graph(rp, ci, bptr)
    rp, ci = g.rp, g.ci
    a = np.asarray(a).astype(dtype)
    lu, s = np.zeros(len(ci), dtype=dtype), np.zeros(len(ci), dtype=dtype)
    d = np.zeros(g.n, dtype=dtype)            # pivots d_i (unscaled diagonal of U)
    kernel = form == "kernel"
    assert form in ("kernel", "textbook")
    for r0, r1 in _blocks(g.bptr):
        nb = r1 - r0
        w, sw = np.zeros(nb, dtype=dtype), np.zeros(nb, dtype=dtype)
        pat = np.zeros(nb, dtype=bool)
        up = {}     # row -> its strict upper in-block part: (local columns, the stored values (U / d), U itself, |U / d|)
        for i in range(r0, r1):
            lo, hi, dg = g.lo[i], g.hi[i], g.diag[i]
            cols = ci[lo:hi] - r0
            pat[cols] = True
            w[cols] = a[lo:hi]
            sw[cols] = np.abs(a[lo:hi])
            skipped = skip_update != i
            for p in range(lo, dg):               # L part, ascending columns
                k = ci[p]
                mult = w[k - r0]
                cu, vu, vraw, au = up[k]
                m = pat[cu]
                if not skipped and len(cu) and m[-1]:   # WRONG: the pivot row's last in-block entry misses this update
                    m = m.copy()
                    m[-1] = False
                    skipped = True
                if kernel:
                    lik = mult * lu[g.diag[k]]          # InV[jj] *= DV[j]
                    w[cu[m]] -= mult * vu[m]            # a_ik (U_kj / d_k)
                else:
                    lik = mult / d[k]
                    w[cu[m]] -= lik * vraw[m]           # (a_ik / d_k) U_kj
                sw[cu[m]] += np.abs(mult) * au[m]       # |l_ik| |u_kj| = |a_ik| |U_kj / d_k|
                w[k - r0] = lik
                sw[k - r0] = sw[k - r0] / np.abs(d[k])
            di = w[i - r0]
            d[i] = di
            dinv = dtype(1) / di
            ucols = ci[dg + 1:hi] - r0
            uvals = w[ucols].copy()
            scaled = uvals * dinv if kernel else uvals / di
            stored = uvals if unscaled_upper == i else scaled
            up[i] = (ucols, stored, uvals, np.abs(scaled))
            lu[lo:dg] = w[cols[:dg - lo]]
            lu[dg] = dinv
            lu[dg + 1:hi] = stored
            s[lo:dg] = sw[cols[:dg - lo]]
            s[dg] = sw[i - r0] / (di * di)
            s[dg + 1:hi] = sw[ucols] / np.abs(di)
            pat[cols] = False
    if cross_block:
        p = g.cross_entry(a)
        lu[p] = a[p] * lu[g.diag[ci[p]]]
    return lu, s


def stream_rounded(g, lu):
    """the factors as the float stream holds them: in-block off-diagonal entries through float, inverse pivots unchanged"""
    out = np.array(lu, dtype=np.float64, copy=True)
    off = g.inside & (g.ci != g.rows)
    out[off] = out[off].astype(np.float32).astype(np.float64)
    return out


def _solve_block(g, lu, x, r0, r1, off, skip_dinv=None, cross=None, width=None):
    """in place on x (rows r0..r1 of the block at x[r0 - off ...], one row of x per matrix row): L, 1/d, U.  width(i): how many leading
    columns of x the forward sweep has to touch in row i (the inverse of a unit lower triangle is lower triangular)."""
    ci = g.ci
    for i in range(r0, r1):
        lo, dg = g.lo[i], g.diag[i]
        if dg > lo:
            c = ci[lo:dg] - off
            if width is None:
                x[i - off] -= lu[lo:dg] @ x[c]
            else:
                x[i - off, :width(i)] -= lu[lo:dg] @ x[c, :width(i)]
        if cross is not None and cross[0] == i:        # WRONG: a coupling to the block in front of this one
            x[i - off] -= cross[2] * x[cross[1] - off]
    dinv = lu[g.diag[r0:r1]]
    if skip_dinv is not None and r0 <= skip_dinv < r1:  # WRONG: one row keeps y instead of y / d
        dinv = dinv.copy()
        dinv[skip_dinv - r0] = 1
    x[r0 - off:r1 - off] = (x[r0 - off:r1 - off].T * dinv).T
    for i in range(r1 - 1, r0 - 1, -1):
        dg, hi = g.diag[i], g.hi[i]
        if hi > dg + 1:
            x[i - off] -= lu[dg + 1:hi] @ x[ci[dg + 1:hi] - off]


def inverses(g, lu):
    """the explicit float64 inverses P_b = U^-1 D^-1 L^-1 of every non-empty block, built column by column from the factors `lu`"""
    out = []
    for r0, r1 in _blocks(g.bptr):
        P = np.eye(r1 - r0)
        _solve_block(g, lu, P, r0, r1, r0, width=lambda i: i - r0 + 1)
        out.append(P)
    return out


def solve(rp, ci, lu, bptr, b, ncomp=1, dtype=LD, mode="sweep", stream_float=False, skip_dinv=None, cross_block=None, graph=None, P=None):
    """x = U^-1 D^-1 L^-1 b per block, ncomp interleaved right-hand sides (b[node * ncomp + c]).  mode "dense" (float64 only): through
    the explicit inverses (P: the result of `inverses` for these factors, built here if not given).  WRONG variants (mode "sweep"):
    skip_dinv = row that misses the D^-1 scaling; cross_block = (row, column, multiplier) of a coupling across a block boundary kept
    in the forward sweep."""
    g = graph or Graph(rp, ci, bptr)
    lu = stream_rounded(g, lu) if stream_float else np.asarray(lu, dtype=np.float64)
    lu = lu.astype(dtype)
    x = np.array(np.asarray(b).reshape(g.n, ncomp), dtype=dtype, copy=True)
    assert mode == "sweep" or (mode == "dense" and dtype == np.float64)
    if mode == "dense":
        for (r0, r1), Pb in zip(_blocks(g.bptr), P if P is not None else inverses(g, lu)):
            x[r0:r1] = Pb @ x[r0:r1]
    else:
        for r0, r1 in _blocks(g.bptr):
            _solve_block(g, lu, x, r0, r1, 0, skip_dinv, cross_block)
    return x.reshape(-1)


def rhs(n, ncomp=1, seed=SEED):
    return np.random.default_rng([seed, n, ncomp]).standard_normal(n * ncomp)


def unit_rhs_rows(bptr):
    """first and last row of the first, a middle and the last non-empty block"""
    blocks = _blocks(bptr)
    picked = [blocks[0], blocks[len(blocks) // 2], blocks[-1]]
    return sorted({r for r0, r1 in picked for r in (r0, r1 - 1)})


class FactorReference:
    """long-double factors of (graph, values, blocks), the scales s_ij, and the float64 restatements' deviation from them"""

    def __init__(self, rp, ci, a, bptr):
        self.g = Graph(rp, ci, bptr)
        self.a = np.asarray(a, dtype=np.float64)
        self.lu, self.s = factor(rp, ci, self.a, bptr, LD, graph=self.g)
        self.inside = self.g.inside
        self.forms = {f: factor(rp, ci, self.a, bptr, np.float64, f, graph=self.g)[0] for f in ("kernel", "textbook")}
        self.err64 = max(self.error(v) for v in self.forms.values())

    def entry_errors(self, lu):
        lu = np.asarray(lu, dtype=np.float64)
        e = np.zeros(len(lu))
        i = self.inside
        # (s_ij = 0: a structural zero no term ever touches, e.g. in a Dirichlet row -- any deviation from 0 is infinitely wrong)
        e[i] = np.asarray(np.abs(lu[i] - self.lu[i]) / np.where(self.s[i] > 0, self.s[i], np.finfo(np.float64).tiny), dtype=np.float64)
        # an entry outside the blocks has no scale of its own (it must be exactly 0): measured against the largest entry of the factor
        e[~i] = np.abs(lu[~i]) / float(np.max(np.abs(self.lu)))
        return e

    def error(self, lu):
        return float(np.max(self.entry_errors(lu)))

    def bound(self, k_margin=None):
        return (K_FACTOR if k_margin is None else k_margin) * (self.err64 + FLOOR)


def compare_factor(ref, lu, k_margin=None):
    """(failures, ratio): the device's factors against the reference, entry by entry"""
    lu = np.asarray(lu, dtype=np.float64)
    if lu.shape != ref.lu.shape:
        return ["factor has shape %s" % (lu.shape,)], 0.0
    if not np.all(np.isfinite(lu)):
        return ["factor not finite"], 0.0
    bound = ref.bound(k_margin)
    assert bound < HARD_LIMIT, bound       # the check itself: no bound may be this loose
    failures = []
    if np.any(lu[~ref.inside] != 0.0):
        failures.append("%d entries outside the blocks are not exactly 0" % int(np.count_nonzero(lu[~ref.inside])))
    e = ref.entry_errors(lu)
    worst = int(np.argmax(e))
    if not e[worst] <= bound:
        failures.append("factor entry %d (row %d, column %d): error %.3e > bound %.3e (err64 %.3e)"
                        % (worst, ref.g.rows[worst], ref.g.ci[worst], e[worst], bound, ref.err64))
    return failures, float(e[worst]) / (ref.err64 + FLOOR)


class Factors:
    """the factors a solve is referred to (the device's own), with their explicit inverses built once for every right-hand side"""

    def __init__(self, g, lu, stream_float=False):
        self.g, self.stream_float = g, stream_float
        self.lu = stream_rounded(g, lu) if stream_float else np.array(lu, dtype=np.float64, copy=True)
        self._P = None

    def P(self):
        if self._P is None:
            self._P = inverses(self.g, self.lu)
        return self._P


class SolveReference:
    """long-double solve of one right-hand side with given factors, and the float64 restatements' deviation from it"""

    def __init__(self, g, lu, b, ncomp, stream_float=False, factors=None):
        f = factors or Factors(g, lu, stream_float)
        self.g, self.ncomp, self.stream_float = g, ncomp, f.stream_float
        self.lu, self.b = f.lu, np.asarray(b, dtype=np.float64)
        args = (g.rp, g.ci, self.lu, g.bptr, self.b, ncomp)
        self.x = solve(*args, dtype=LD, graph=g)
        scale = np.zeros(g.n, dtype=LD)
        ax = np.max(np.abs(self.x.reshape(g.n, ncomp)), axis=1)
        for r0, r1 in _blocks(g.bptr):
            scale[r0:r1] = np.max(ax[r0:r1])
        scale[scale == 0] = 1
        self.scale = np.repeat(scale, ncomp)
        self.err64 = max(self.error(solve(*args, dtype=np.float64, graph=g)), self.error(solve(*args, dtype=np.float64, mode="dense", graph=g, P=f.P())))

    def error(self, x):
        return float(np.max(np.abs(np.asarray(x, dtype=np.float64) - self.x) / self.scale))

    def bound(self, k_margin=None):
        return (K_SOLVE if k_margin is None else k_margin) * (self.err64 + FLOOR)


def compare_solve(ref, x, k_margin=None):
    x = np.asarray(x, dtype=np.float64)
    if x.shape != ref.x.shape:
        return ["x has shape %s" % (x.shape,)], 0.0
    if not np.all(np.isfinite(x)):
        return ["x not finite"], 0.0
    bound = ref.bound(k_margin)
    assert bound < HARD_LIMIT, bound
    e = ref.error(x)
    failures = []
    if not e <= bound:
        k = int(np.argmax(np.abs(x - ref.x) / ref.scale))
        failures.append("x[%d] (row %d): error %.3e > bound %.3e (err64 %.3e)" % (k, k // ref.ncomp, e, bound, ref.err64))
    return failures, e / (ref.err64 + FLOOR)


def block_ptr(n, size):
    """uniform blocks of `size` rows plus the remainder"""
    return np.array(list(range(0, n, size)) + [n], dtype=np.int32)


def split_ptr(n, first):
    """one block of `first` rows, the remainder as a second block"""
    return np.array([0, first, n] if first < n else [0, n], dtype=np.int32)


def ragged_ptr(n, size=85, head=(0, 1, 2, 15, 16, 17, 0, 63, 64, 65), tail_empty=True):
    """an empty block in front, in the middle and at the end; blocks of 1, 2, 15, 16, 17, 63, 64, 65 rows; then `size`-row blocks"""
    ptr = np.cumsum((0,) + tuple(head))
    assert ptr[-1] < n
    out = list(ptr) + list(range(int(ptr[-1]) + size, n, size)) + [n]
    if tail_empty:
        out.append(n)
    return np.array(out, dtype=np.int32)
