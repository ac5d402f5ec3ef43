"""Extended-precision reference of the Schur-complement CG (csrc/nsx_cg.hip, cg() in csrc/nsx_solve.hip), the yardstick it is measured
with, and the comparisons the GPU tests call (tests/test_gpu_schur_cg.py; checked on the CPU by tests/test_cg_reference.py).  A plain
helper module, no fixtures.

The solve is deal.II's SolverCG::solve with a preconditioner, restated by `cg`:
    g = A x - b ; check(0, |g|) ; h = P g ; d = -h ; gh = g.h
    loop: it++ ; Ad ; alpha = gh / d.Ad ; x += alpha d ; g += alpha Ad ; res = |g| ; check(it, res) ; h = P g ; beta = g.h / gh ; d = beta d - h
    check: success if res <= tol, failure if it >= maxiter or NaN ; tol = rtol |b|
A = negative_S_tilde as a CSR matrix; P = the block-Jacobi ILU(0) solve in Ifpack's storage (strict lower = L, diagonal = 1/d, strict
upper = U/d), every block restricted to its own rows and columns.  The data are the DEVICE's own (Nsx.schur(), Nsx.ilu(1), its block
pointer): the comparison isolates the CG (the factors are compared with the oracle elsewhere).

* `reference(op, guess)`: the chain in np.longdouble (x87 extended, eps 1.08e-19) for maxiter = KMAX with every iterate x_k and residual
  res_k kept, AND the same chain in float64 twice -- with the triangular solves, and with explicit block inverses P_b built column by
  column from the factors (what the dense kernels apply).  err64[k], the running maximum over iterations <= k of the deviation of BOTH
  float64 chains from the extended one, is the yardstick: what a correct implementation in the kernels' number format loses on this input.
* `compare(ref, k, x, last)`: an iterate and its residual against x_k / res_k, each with the bound K * (err64[k] + FLOOR), FLOOR = 4 eps.

Scales:
  x_k    entry by entry, relative to max |x_k| of the reference
  res_k  relative to |b|, NOT to itself: the recursively updated residual carries an absolute error (the two float64 chains differ from
         each other by far more than eps relative to res_30 while both are below 1e-17 of |b|)

K is the margin for another, equally valid grouping of the sums (per lane group, wave, block, grid, partial-sum array, fold): 10 x the
largest ratio error / (err64 + FLOOR) measured on the MI355X over every case of tests/test_gpu_schur_cg.py, rounded up -- see K below.
No asserted bound may reach HARD_LIMIT = 1e-11 (asserted in compare)."""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended-precision long double (x87: eps 1.08e-19)"
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS

# Margin over the float64 chains' own deviation.  Largest ratios  error / (err64[k] + FLOOR)  measured on the MI355X over every
# configuration x path x guess x call of tests/test_gpu_schur_cg.py (recorded as "schur_cg_unit"), x_k / res_k:
#   k_cg_schur<6,true> / <6,false>  1.94 / 1.96 (both on the ragged layout)     <8,true> / <8,false>  1.12 / 0.70
#   <0,false> two register sets  1.12 / 0.85     <0,false> one wide set  1.25 / 0.86
#   two launches per iteration  1.25 / 0.85, with ncclAllReduce  0.79 / 0.85, with folded partial sums (3D level 2, 2-row blocks)  0.33 / 0.36
#   cg() with explicit inverses  0.43 / 0.61, with triangular solves  0.95 / 0.51
#   two processes (k_cgd_pack)  0.36 / 0.48
#   k_cg_schur<6,true> near the unique-column limit (3D level 2, 96-row blocks)  0.92 / 0.49
# -- the variants of one block size give the same numbers: register- or LDS-resident operands change no sum.
# K = 10 x the largest (1.96), rounded up; K_DIST the same rule on the two-process leg (0.48).  With them the largest asserted bound
# is far below HARD_LIMIT wherever a threshold or an iterate is placed (see stops()).
K = 20.0
K_DIST = 5.0      # the two-process leg (its Schur products are summed in another order than the single-process handle's the reference is built from)
HARD_LIMIT = 1e-11

KMAX = 60                    # iterations of the reference chain; x_KMAX is "the solution" the guesses are scaled with
STOP_KMAX = 50               # stopping thresholds are placed at record lows of the residual up to this iteration
ITERATES = (0, 1, 2, 3, 5, 8, 13, 21, 30)
SEED = 2025
GUESSES = ("zero", "visible", "exact")


def _psum(x):
    return np.sum(x)  # numpy's pairwise summation


class Operator:
    """negative_S_tilde (CSR) and its block-Jacobi ILU(0) factors on the same graph, in the numbering the solve runs in.  Hashable by
    identity: `reference` caches per Operator."""

    def __init__(self, rowptr, colind, values, lu, block_ptr):
        self.rp, self.ci = np.asarray(rowptr, dtype=np.int64), np.asarray(colind, dtype=np.int64)
        self.sv, self.lu = np.asarray(values, dtype=np.float64), np.asarray(lu, dtype=np.float64)
        self.bptr = np.asarray(block_ptr, dtype=np.int64)
        self.n = n = len(self.rp) - 1
        assert self.bptr[0] == 0 and self.bptr[-1] == n and np.all(np.diff(self.bptr) > 0) and np.all(np.diff(self.rp) > 0)
        rows = np.repeat(np.arange(n), np.diff(self.rp))
        assert np.all(np.diff(self.ci)[np.diff(rows) == 0] > 0), "columns must ascend within a row"
        blk = np.searchsorted(self.bptr, np.arange(n), side="right") - 1
        r0, r1 = self.bptr[blk][rows], self.bptr[blk + 1][rows]
        inside = (self.ci >= r0) & (self.ci < r1)
        self._low = [np.flatnonzero(inside[a:b] & (self.ci[a:b] < i)) + a for i, (a, b) in enumerate(zip(self.rp[:-1], self.rp[1:]))]
        self._up = [np.flatnonzero(inside[a:b] & (self.ci[a:b] > i)) + a for i, (a, b) in enumerate(zip(self.rp[:-1], self.rp[1:]))]
        self._diag = np.flatnonzero(self.ci == rows)
        assert len(self._diag) == n
        # the strongest coupling to a row of an EARLIER block (a broken restatement keeps it in the forward solve).  The factors hold
        # zeros outside the blocks; the multiplier such a coupling would carry is, to first order, S_ij / S_jj
        across = np.flatnonzero(self.ci < r0)
        self.cross_entry = int(across[np.argmax(np.abs(self.sv[across]))]) if len(across) else None
        self.cross_row = int(rows[self.cross_entry]) if len(across) else None
        self.cross_value = float(self.sv[self.cross_entry] * self.lu[self._diag[self.ci[self.cross_entry]]]) if len(across) else 0.0
        self._cache = {}

    def _prepared(self, dtype):
        if dtype not in self._cache:
            lu = self.lu.astype(dtype)
            self._cache[dtype] = (self.sv.astype(dtype), lu[self._diag],
                                  [(self.ci[k], lu[k]) for k in self._low], [(self.ci[k], lu[k]) for k in self._up])
        return self._cache[dtype]

    def apply(self, x, dtype, drop_tail=None):
        """A x, rows summed over the CSR product; drop_tail = a row whose last entry is left out (a WRONG product)"""
        prod = self._prepared(dtype)[0] * x[self.ci]
        if drop_tail is not None:
            prod[self.rp[drop_tail + 1] - 1] = 0
        return np.add.reduceat(prod, self.rp[:-1])

    def _solve_block(self, x, r0, r1, off, dtype, cross=False):
        """in place on x (rows r0..r1 of the block sit at x[r0 - off ...]; one or several right-hand sides): L, 1/d, U"""
        _, diag, low, up = self._prepared(dtype)
        for i in range(r0, r1):
            c, v = low[i]
            if len(c):
                x[i - off] -= v @ x[c - off]
            if cross and i == self.cross_row:  # WRONG: a coupling to the block in front of this one
                x[i - off] -= dtype(self.cross_value) * x[self.ci[self.cross_entry] - off]
        x[r0 - off:r1 - off] = (x[r0 - off:r1 - off].T * diag[r0:r1]).T
        for i in range(r1 - 1, r0 - 1, -1):
            c, v = up[i]
            if len(c):
                x[i - off] -= v @ x[c - off]

    def solve(self, g, dtype=np.float64, cross_block=False):
        """h = P g by the triangular solves, block by block"""
        x = np.array(g, dtype=dtype, copy=True)
        for r0, r1 in zip(self.bptr[:-1], self.bptr[1:]):
            self._solve_block(x, r0, r1, 0, dtype, cross_block)
        return x

    def inverses(self):
        """the explicit float64 inverses P_b = U^-1 D^-1 L^-1, built column by column from the factors"""
        if "inv" not in self._cache:
            out = []
            for r0, r1 in zip(self.bptr[:-1], self.bptr[1:]):
                X = np.eye(r1 - r0)
                self._solve_block(X, r0, r1, r0, np.float64)
                out.append(X)
            self._cache["inv"] = out
        return self._cache["inv"]

    def dense(self, g):
        h = np.empty_like(g)
        for P, r0, r1 in zip(self.inverses(), self.bptr[:-1], self.bptr[1:]):
            h[r0:r1] = P @ g[r0:r1]
        return h


class Solve:
    """what one call of the solver returns, plus (history=True) every iterate and residual"""

    def __init__(self, x, steps, last, status, xs=None, res=None):
        self.x, self.steps, self.last, self.status, self.xs, self.res = x, steps, last, status, xs, res

    def out(self):
        """as Nsx.schur_cg returns it"""
        return np.asarray(self.x, dtype=np.float64), self.steps, float(self.last), self.status


def cg(op, x0, b, rtol, maxiter, dtype, precond="tri", history=False, beta_gg=False, stale_gh=False, plus_h=False, tol_g0=False,
       stop_gh=False, extra_update=False, drop_tail=None, cross_block=False, stale_h=None):
    """SolverCG::solve in `dtype`; precond "tri" (triangular solves) or "dense" (explicit float64 inverses).  The other keyword arguments
    restate the solve WRONGLY (tests/test_cg_reference.py: the comparisons must notice each of them): beta_gg = beta from g.g;
    stale_gh = alpha with the g.h of the iteration before; plus_h = d = beta d + h; tol_g0 = tolerance from |g_0|; stop_gh = the stop
    test on sqrt(g.h); extra_update = one more update of x after the converging iteration; drop_tail = row whose last entry is left
    out of A d; cross_block = one coupling across a block boundary kept in P; stale_h = row whose h keeps its previous value."""
    x, b = np.asarray(x0).astype(dtype), np.asarray(b).astype(dtype)

    def P(g):
        return op.solve(g, dtype, cross_block) if precond == "tri" else op.dense(g)

    def dot(a, c):
        return _psum(a * c)

    def check(it, value):
        if value <= tol:
            return 1
        return 2 if (it >= maxiter or np.isnan(value)) else 0

    g = op.apply(x, dtype) - b
    res = np.sqrt(dot(g, g))
    tol = dtype(rtol) * (res if tol_g0 else np.sqrt(dot(b, b)))
    h = P(g)
    gh = dot(g, h)
    gg = dot(g, g)
    xs, rs = [x.copy()], [res]
    it = 0
    conv = check(0, np.sqrt(abs(gh)) if stop_gh else res)
    if conv == 0:
        d, gh_before = -h, gh
        while True:
            it += 1
            Ad = op.apply(d, dtype, drop_tail)
            alpha = (gh_before if stale_gh else gh) / dot(d, Ad)
            x = x + alpha * d
            g = g + alpha * Ad
            res = np.sqrt(dot(g, g))
            h_old, h = h, P(g)
            if stale_h is not None:
                h[stale_h] = h_old[stale_h]
            gh_new, gg_new = dot(g, h), dot(g, g)
            if history:
                xs.append(x.copy())
                rs.append(res)
            conv = check(it, np.sqrt(abs(gh_new)) if stop_gh else res)
            beta = gg_new / gg if beta_gg else gh_new / gh
            d = beta * d + h if plus_h else beta * d - h
            gh_before, gh, gg = gh, gh_new, gg_new
            if conv:
                if extra_update and conv == 1:
                    x = x + (gh / dot(d, op.apply(d, dtype))) * d
                break
    return Solve(x, it, res, 0 if conv == 1 else 1, xs if history else None, np.array(rs, dtype=dtype) if history else None)


def rhs(n, seed=SEED):
    return np.random.default_rng([seed, n]).standard_normal(n)


class Reference:
    """Extended-precision iterates and residuals of one (operator, right-hand side, guess), and the float64 chains' deviation from them."""

    def __init__(self, op, b, x0, kmax=KMAX):
        self.op, self.b, self.x0, self.kmax = op, np.asarray(b, dtype=np.float64), np.asarray(x0, dtype=np.float64), kmax
        ld = cg(op, self.x0, self.b, 0.0, kmax, LD, history=True)
        self.xs, self.res = ld.xs, ld.res
        self.bnorm = np.sqrt(_psum(self.b.astype(LD) ** 2))
        self.kmax = len(self.xs) - 1
        self.scale = [np.max(np.abs(x)) for x in self.xs]
        if self.scale[0] == 0 and self.kmax >= 1:
            self.scale[0] = self.scale[1]   # (a zero guess: the device has to return it bit for bit anyway)
        ex, er = np.zeros(self.kmax + 1), np.zeros(self.kmax + 1)
        for precond in ("tri", "dense"):
            c = cg(op, self.x0, self.b, 0.0, kmax, np.float64, precond, history=True)
            assert len(c.xs) == len(self.xs)
            for k in range(self.kmax + 1):
                ex[k] = max(ex[k], float(np.max(np.abs(c.xs[k] - self.xs[k])) / self.scale[k]))
                er[k] = max(er[k], float(abs(c.res[k] - self.res[k]) / self.bnorm))
        self.err64_x, self.err64_res = np.maximum.accumulate(ex), np.maximum.accumulate(er)

    def rel_res(self):
        return np.asarray(self.res / self.bnorm, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def reference(op, guess="zero"):
    """The reference of `op` with b = rhs(op.n) and the guess "zero", "visible" (x_ref (1 + 0.5 xi), x_ref = iterate KMAX from the zero
    guess, xi seeded standard normal: a guess has to be scaled with the solution to leave a trace in the residuals) or "exact"
    (float64(x_ref): converged before the first iteration; only res_0 is needed)."""
    b = rhs(op.n)
    if guess == "zero":
        return Reference(op, b, np.zeros(op.n))
    x_ref = np.asarray(reference(op, "zero").xs[KMAX], dtype=np.float64)
    if guess == "visible":
        return Reference(op, b, x_ref * (1 + 0.5 * np.random.default_rng([SEED, op.n, 1]).standard_normal(op.n)))
    if guess == "exact":
        return Reference(op, b, x_ref, kmax=0)
    raise ValueError(guess)


def stops(ref, with_reference_rtol=True):
    """[(rtol, steps the reference takes)]: thresholds sqrt(runmin_{k-1} res_k) / |b| at the iterations k <= STOP_KMAX where the
    residual sets a record low at least 1 % below the previous one, and the reference's own rtol = 1e-2 where every residual of the
    chain stays 1 % clear of it.  A threshold is only placed where it is further from both residuals it separates than 10 x the
    bound asserted for a residual (bounds(): relative to |b|) with the larger of the two margins: below that -- residuals of 1e-12 |b|
    and less, which these solves reach within the 50 iterations -- a correct float64 solve may stop a step earlier or later.
    Nor is one placed at an iteration whose bounds would reach HARD_LIMIT: where the residual stagnates for twenty iterations (the 3D
    level-2 cylinder in 96-row blocks, zero guess: 4.5e-2 |b| from iteration 13 to 40) ANY float64 CG leaves the exact recurrence --
    both float64 chains are 2e-12 of max |x_k| away from the extended one at iteration 45 (4e-15 at 30), so 10 x that is no bound on a
    kernel any more; there the thresholds up to iteration 17 remain (the iterates are compared up to 30 in every configuration)."""
    r = ref.rel_res()
    out, runmin = [], r[0]
    for k in range(1, min(STOP_KMAX, ref.kmax) + 1):
        if r[k] < 0.99 * runmin:
            thr = float(np.sqrt(runmin * r[k]))
            if min(runmin - thr, thr - r[k]) > 10 * bounds(ref, k, max(K, K_DIST))[1] and max(bounds(ref, k, max(K, K_DIST))) < HARD_LIMIT:
                out.append((thr, k))
        runmin = min(runmin, r[k])
    hit = np.flatnonzero(r <= 1e-2)
    if with_reference_rtol and len(hit) and np.all(np.abs(r / 1e-2 - 1) >= 0.01) and max(bounds(ref, int(hit[0]), max(K, K_DIST))) < HARD_LIMIT:
        out.append((1e-2, int(hit[0])))
    return out


def bounds(ref, k, k_margin=None):
    k_margin = K if k_margin is None else k_margin
    return k_margin * (ref.err64_x[k] + FLOOR), k_margin * (ref.err64_res[k] + FLOOR)


def compare(ref, k, x, last, k_margin=None):
    """iterate and residual of a solve that made k steps against x_k / res_k.  Returns (failures, ratios): messages, empty when every
    assertion holds, and error / (bound / K) per quantity, the numbers K is fixed from."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape != (ref.op.n,):
        return ["x has shape %s" % (x.shape,)], {}
    if not (np.all(np.isfinite(x)) and np.isfinite(last)):
        return ["x or the residual not finite"], {}
    if not 0 <= k <= ref.kmax:
        return ["%d steps: beyond the reference's %d" % (k, ref.kmax)], {}
    bx, br = bounds(ref, k, k_margin)
    assert bx < HARD_LIMIT and br < HARD_LIMIT, (k, bx, br)   # the check itself: no bound may be this loose
    k_used = K if k_margin is None else k_margin
    ex = float(np.max(np.abs(x - ref.xs[k])) / ref.scale[k])
    er = float(abs(LD(last) - ref.res[k]) / ref.bnorm)
    failures = []
    if not ex <= bx:
        failures.append("x_%d: error %.3e > bound %.3e (err64 %.3e)" % (k, ex, bx, ref.err64_x[k]))
    if not er <= br:
        failures.append("res_%d: error %.3e > bound %.3e (err64 %.3e)" % (k, er, br, ref.err64_res[k]))
    return failures, {"x": ex / (bx / k_used), "res": er / (br / k_used)}


def check_iterate(ref, k, out, k_margin=None):
    """a call with rtol = 0, maxiter = k from the reference's guess: status 1 after exactly k steps, x_k and res_k; k = 0 returns
    the guess bit for bit"""
    x, steps, last, status = out
    failures = []
    if status != 1 or steps != k:
        failures.append("status %d after %d steps, expected 1 after %d" % (status, steps, k))
    if k == 0 and not np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64), ref.x0.view(np.uint64)):
        failures.append("maxiter = 0 changed x")
    f, ratios = compare(ref, k, x, last, k_margin)
    return failures + f, ratios


def check_stop(ref, rtol, steps_ref, out, k_margin=None):
    """a call with the tolerance rtol |b|: status 0 after EXACTLY the reference's steps, and the iterate of that step (not the next)"""
    x, steps, last, status = out
    failures = []
    if status != 0 or steps != steps_ref:
        failures.append("status %d after %d steps, expected 0 after %d" % (status, steps, steps_ref))
    if steps_ref == 0 and not np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64), ref.x0.view(np.uint64)):
        failures.append("a solve that was converged at step 0 changed x")
    f, ratios = compare(ref, steps_ref, x, last, k_margin)
    return failures + f, ratios


def check_zero_rhs(out):
    """b = 0, x0 = 0: converged at step 0, x all zeros, nothing non-finite"""
    x, steps, last, status = out
    failures = []
    if status != 0 or steps != 0:
        failures.append("b = 0: status %d after %d steps" % (status, steps))
    if not np.isfinite(last) or last != 0:
        failures.append("b = 0: residual %r" % last)
    if not (np.all(np.isfinite(x)) and not np.any(x)):
        failures.append("b = 0: x is not all zeros")
    return failures


def schedule(ref_zero, ref_visible, ref_exact):
    """every call of one configuration: (kind, guess, rtol, maxiter, expected steps); kinds "iterate", "stop", "exact" (the last where
    float64(x_ref) IS converged for rtol = 1e-2: with 2-row blocks on the 3D level-2 cylinder iterate KMAX still has 5.6e-2 |b|)"""
    calls = []
    for guess, ref in (("zero", ref_zero), ("visible", ref_visible)):
        calls += [("iterate", guess, 0.0, k, k) for k in ITERATES]
        calls += [("stop", guess, rtol, 100000, k) for rtol, k in stops(ref)]
    if ref_exact.rel_res()[0] < 0.99e-2:
        calls.append(("exact", "exact", 1e-2, 100000, 0))
    return calls


def block_ptr(n, size):
    """uniform blocks of `size` rows plus the remainder"""
    return np.array(list(range(0, n, size)) + [n], dtype=np.int32)


def ragged_ptr(n, size=96):
    """blocks of 1, 2, 15, 16, 17, 31, 33, 64, 95 and 96 rows, then `size`-row blocks: block tails, one-row blocks and full blocks in one grid"""
    head = np.cumsum([0, 1, 2, 15, 16, 17, 31, 33, 64, 95, 96])
    assert head[-1] < n
    return np.array(list(head) + list(range(int(head[-1]) + size, n, size)) + [n], dtype=np.int32)


def to_internal(rowptr, colind, values, perm):
    """CSR values on a graph in the caller's numbering -> the numbering `perm` (caller node -> internal node) leads to: rows and columns
    through perm, columns sorted"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    r2, c2 = np.asarray(perm)[rows], np.asarray(perm)[np.asarray(colind, dtype=np.int64)]
    k = np.lexsort((c2, r2))
    rp2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r2, minlength=n), out=rp2[1:])
    return rp2, c2[k], np.asarray(values, dtype=np.float64)[k]
