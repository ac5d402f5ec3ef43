"""Extended-precision reference of the GMRES driver (gmres() in csrc/nsx_solve.hip), the yardstick it is measured with, and the
comparisons the GPU tests call (tests/test_gpu_gmres.py; checked on the CPU by tests/test_gmres_reference.py).  A plain helper module.

The solve is deal.II's SolverGMRES::solve as gmres() restates it, restated once more by `gmres`:
    cycle:  v_0 = P (b - A x) ; rho = |v_0| ; check(steps, rho) -- the TRUE preconditioned residual ; v_0 /= rho ; gamma_0 = rho
      inner = 0 .. 27:  steps++ ; vv = P A v_inner ; modified Gram-Schmidt against v_0 .. v_inner: h_i = vv . v_i, vv -= h_i v_i ; s = |vv|
        on inner % 5 == 4, unless the solve already re-orthogonalises: if not s > 10 |vv before the sweep| sqrt(eps), EVERY iteration of the
        solve from here on sweeps a second time: h += h2, s = |vv| after the second sweep
        v_{inner+1} = vv / s ; Givens rotations on the column, gamma_{inner+1} = -s_i gamma_inner, gamma_inner *= c_i
        check(steps, |gamma_{inner+1}|) -- the ESTIMATE
      x += sum_i y_i v_i with H y = gamma by back-substitution; next cycle unless the check ended the solve
    check: success if value <= tol, failure if steps >= maxiter or NaN
So last_residual is the estimate |gamma| when the solve ends inside a cycle and the true residual when it ends at a restart (or at once).
A = negative_S_tilde, P = its block-Jacobi ILU(0), both the DEVICE's own data in a cg_reference.Operator (Nsx.schur(), Nsx.ilu(1)): the
comparison isolates the driver.

* `Reference(op, b, x0)`: the chain in np.longdouble for KMAX steps with every iterate x_k, every estimate and every restart residual
  kept, AND the same chain in float64 twice: dot products summed pairwise (numpy) and sequentially, the second one with the explicit
  block inverses for P.  err64[k], the running maximum over steps <= k of the deviation of both float64 chains from the extended one,
  is the yardstick, exactly as in cg_reference: bound = K (err64[k] + 4 eps), K = cg_reference.K = 20 (the margin for another valid
  grouping of the sums, not tuned to these kernels), x_k entry by entry relative to max |x_k|, residuals relative to |P b|.
  No asserted bound may reach cg_reference.HARD_LIMIT = 1e-11 (asserted in compare).
* `iterates(ref)`: the steps of ITERATES whose bounds stay below HARD_LIMIT on the CPU; `stops(ref)`: thresholds between two record lows
  of the sequence of checked values, each with the step the reference stops at and whether the restart's true residual met it first.

Iterates kept (chosen on the CPU by iterates(), asserted in tests/test_gmres_reference.py): all of ITERATES on the 745-row and on the
366-row Schur system from the zero guess and from the scaled guess (err64 of x_k at most 1.1e-13 through step 57, 4.1e-14 on the 3D mesh).
Largest ratios error / (err64 + 4 eps) measured on the MI355X over tests/test_gpu_gmres.py (recorded as "gmres_unit"), x_k / checked value:
Schur iterates 1.84 / 1.44, stopping steps 1.84 / 1.44, velocity iterates 0.37 / 0.30, re-orthogonalising solve 0.47 / 0.32 -- none above K / 10.
* `nearly_invariant_rhs` / `reorth_reference`: the case on which SolverGMRES really re-orthogonalises (s / |vv| = 5e-9 at step 5).
* `VelocityOperator` / `velocity_reference`: F on the scalar P2 graph with its block-Jacobi ILU(0) through ilu_reference; all of
  VELOCITY_ITERATES are kept on the 8-subdomain configuration (err64 5e-15 through the restart).
MUTANTS lists seven wrong restatements.  Four are rejected (tests/test_gmres_reference.py).  h2_omitted, norm_of_first_sweep and
no_restart_residual change a correct solve by less than a third of the bound even on the nearly invariant case, for the reason that
file's test_what_the_second_sweep_changes_is_of_rounding_size states and measures."""
import functools

import numpy as np

import cg_reference as C

LD = C.LD
EPS, FLOOR, K, HARD_LIMIT = C.EPS, C.FLOOR, C.K, C.HARD_LIMIT
RESTART = 28                  # KRYLOV_N_TMP - 2 iterations per cycle
ITERATES = (0, 1, 2, 3, 5, 8, 13, 21, 27, 28, 29, 33, 56, 57)
KMAX = 60
SEED = 2026
MUTANTS = ("no_restart_residual", "h2_omitted", "norm_of_first_sweep", "givens_sign", "x0_ignored", "second_cycle_overwrites", "tol_b_squared")


def _dot(kind):
    if kind == "pairwise":
        return lambda a, c: np.sum(a * c)
    return lambda a, c: np.cumsum(a * c)[-1]      # one term after the other


class Solve:
    def __init__(self, x, steps, last, status, xs, est, true, reorth_from):
        self.x, self.steps, self.last, self.status = x, steps, last, status
        self.xs, self.est, self.true, self.reorth_from = xs, est, true, reorth_from


def gmres(op, x0, b, tol, maxiter, dtype, dots="pairwise", precond="tri", rtol=None, mutant=None, force_reorth=False, trace=False):
    """SolverGMRES::solve in `dtype`.  tol absolute, or rtol: tol = rtol |b|.  Keeps xs[k] (the iterate a solve that ends at step k
    returns), est[k] (|gamma| checked at step k >= 1), true[k] (the true residual checked at step k = 0, 28, 56, ...), reorth_from (the
    first step that swept twice, or None).  mutant: one of MUTANTS, a WRONG restatement.  force_reorth: sweep twice from step 5 on."""
    assert mutant is None or mutant in MUTANTS
    dot = _dot(dots)
    x, b = np.asarray(x0).astype(dtype), np.asarray(b).astype(dtype)
    n = len(b)

    def P(g):
        return op.solve(g, dtype) if precond == "tri" else op.dense(g)

    def check(step, value):
        if value <= tol:
            return 1
        return 2 if (step >= maxiter or np.isnan(value)) else 0

    if rtol is not None:
        bb = dot(b, b)
        tol = dtype(rtol) * (bb if mutant == "tol_b_squared" else np.sqrt(bb))
    xs, est, true = {}, {}, {}
    steps, state, re_orth, reorth_from, last = 0, 0, False, None, dtype(0)
    sqrt_eps = np.sqrt(dtype(2.220446049250313e-16))
    carried, ratio5 = None, None
    first_cycle = True
    while True:
        v0 = P(b - op.apply(x, dtype))
        rho = np.sqrt(dot(v0, v0))
        if mutant == "no_restart_residual" and carried is not None:
            rho = carried
        true[steps], last = rho, rho
        xs.setdefault(steps, x.copy())
        state = check(steps, rho)
        if state != 0:
            break
        V = np.zeros((RESTART + 1, n), dtype=dtype)
        V[0] = v0 / rho
        H = np.zeros((RESTART + 1, RESTART), dtype=dtype)
        gamma = np.zeros(RESTART + 1, dtype=dtype)
        gamma[0] = rho
        ci, si = np.zeros(RESTART, dtype=dtype), np.zeros(RESTART, dtype=dtype)
        x_start, dim = x.copy(), 0
        for inner in range(RESTART):
            steps += 1
            vv = P(op.apply(V[inner], dtype))
            dim = inner + 1
            consider = (not re_orth) and inner % 5 == 4
            before = np.sqrt(dot(vv, vv)) if consider else None
            hh = np.zeros(dim + 1, dtype=dtype)
            for i in range(dim):
                hh[i] = dot(vv, V[i])
                vv = vv - hh[i] * V[i]
            s = np.sqrt(dot(vv, vv))
            if consider and steps == 5:
                ratio5 = s / before
            if consider and (force_reorth or not s > 10 * before * sqrt_eps):
                re_orth = True
            if re_orth:
                if reorth_from is None:
                    reorth_from = steps
                s_first = s
                for i in range(dim):
                    h2 = dot(vv, V[i])
                    vv = vv - h2 * V[i]
                    if mutant != "h2_omitted":
                        hh[i] += h2
                s = np.sqrt(dot(vv, vv))
                if mutant == "norm_of_first_sweep":
                    s = s_first
            hh[dim] = s
            if s != 0:
                V[dim] = vv / s
            for i in range(inner):
                t = hh[i]
                hh[i] = ci[i] * t + si[i] * hh[i + 1]
                hh[i + 1] = -si[i] * t + ci[i] * hh[i + 1]
            r = 1 / np.sqrt(hh[inner] * hh[inner] + hh[inner + 1] * hh[inner + 1])
            si[inner], ci[inner] = hh[inner + 1] * r, hh[inner] * r
            hh[inner] = ci[inner] * hh[inner] + si[inner] * hh[inner + 1]
            gamma[inner + 1] = (si[inner] if mutant == "givens_sign" else -si[inner]) * gamma[inner]
            gamma[inner] *= ci[inner]
            H[:dim, inner] = hh[:dim]
            rho = abs(gamma[dim])
            est[steps], last = rho, rho
            # the iterate a solve ending here returns
            y = np.zeros(dim, dtype=dtype)
            for i in range(dim - 1, -1, -1):
                y[i] = (gamma[i] - H[i, i + 1:dim] @ y[i + 1:]) / H[i, i]
            upd = np.zeros(n, dtype=dtype)
            for i in range(dim):
                upd = upd + y[i] * V[i]
            start = x_start
            if (mutant == "x0_ignored" and first_cycle) or (mutant == "second_cycle_overwrites" and not first_cycle):
                start = np.zeros(n, dtype=dtype)
            xs[steps] = start + upd
            state = check(steps, rho)
            if state != 0:
                break
        x = xs[steps]
        carried = rho
        first_cycle = False
        if state != 0:
            break
    out = Solve(x, steps, last, 0 if state == 1 else 1, xs, est, true, reorth_from)
    out.ratio5 = None if ratio5 is None else float(ratio5)      # s / |vv| of SolverGMRES' test at step 5
    return out


class VelocityOperator:
    """F on the scalar P2 graph (one entry serves the dim interleaved components) and its block-Jacobi ILU(0) in Ifpack's storage, with
    the interface gmres() uses of a cg_reference.Operator: the device's own exported F (rounded through float for NSX_INNER_FP32, as
    the float stream of the factors' off-diagonal entries is) and Nsx.ilu(0), applied through ilu_reference."""

    def __init__(self, rp, ci, F, lu, node_ptr, dim, fp32=False):
        import ilu_reference as I
        self._I, self.dim, self.fp32 = I, dim, fp32
        self.g = I.Graph(rp, ci, node_ptr)
        self.rp, self.ci = self.g.rp, self.g.ci
        self.F = np.asarray(F, dtype=np.float64)
        if fp32:
            self.F = self.F.astype(np.float32).astype(np.float64)
        self.lu = I.stream_rounded(self.g, lu) if fp32 else np.asarray(lu, dtype=np.float64)
        self.n = (len(self.rp) - 1) * dim
        self.perm = None

    def apply(self, x, dtype):
        X = np.asarray(x, dtype=dtype).reshape(-1, self.dim)
        return np.add.reduceat(self.F.astype(dtype)[:, None] * X[self.ci], self.rp[:-1], axis=0).reshape(-1)

    def solve(self, g, dtype=np.float64):
        return self._I.solve(self.rp, self.ci, self.lu, self.g.bptr, g, ncomp=self.dim, dtype=dtype, graph=self.g)

    dense = None      # no explicit inverses: the second float64 chain differs from the first in the grouping of the dot products alone


VELOCITY_ITERATES = tuple(k for k in (0, 1, 2, 3, 5, 8, 13, 21, 27, 28, 29, 33))
VELOCITY_KMAX = 33


def rhs(n, seed=SEED):
    return np.random.default_rng([seed, n]).standard_normal(n)


class Reference:
    """Extended-precision iterates and checked values of one (operator, right-hand side, guess), and the float64 chains' deviation"""

    def __init__(self, op, b, x0, kmax=KMAX, force_reorth=False):
        self.op, self.b, self.x0 = op, np.asarray(b, dtype=np.float64), np.asarray(x0, dtype=np.float64)
        self.force_reorth = force_reorth
        ld = gmres(op, self.x0, self.b, 0.0, kmax, LD, force_reorth=force_reorth)
        self.ld, self.kmax = ld, ld.steps
        self.xs, self.est, self.true, self.reorth_from = ld.xs, ld.est, ld.true, ld.reorth_from
        pb = op.solve(self.b.astype(LD), LD)
        self.pbnorm = np.sqrt(np.sum(pb * pb))
        self.bnorm = np.sqrt(np.sum(self.b.astype(LD) ** 2))
        self.scale = {k: np.max(np.abs(x)) for k, x in self.xs.items()}
        if self.scale[0] == 0 and self.kmax >= 1:
            self.scale[0] = self.scale[1]
        ex, er = np.zeros(self.kmax + 1), np.zeros(self.kmax + 1)
        self.chains = []
        for dots, precond in (("pairwise", "tri"), ("sequential", "dense" if op.dense is not None else "tri")):
            c = gmres(op, self.x0, self.b, 0.0, kmax, np.float64, dots, precond, force_reorth=force_reorth)
            assert c.steps == ld.steps
            self.chains.append(c)
            for k in range(self.kmax + 1):
                ex[k] = max(ex[k], float(np.max(np.abs(c.xs[k] - self.xs[k])) / self.scale[k]))
                for mine, theirs in ((c.est, self.est), (c.true, self.true)):
                    if k in theirs:
                        er[k] = max(er[k], float(abs(mine[k] - theirs[k]) / self.pbnorm))
        self.err64_x, self.err64_res = np.maximum.accumulate(ex), np.maximum.accumulate(er)

    def last(self, k, at_restart=False):
        """what a solve that ends at step k reports: the estimate, or the true residual if it ends at the restart's check (or at step 0)"""
        return self.true[k] if (at_restart or k == 0) else self.est[k]

    def checks(self):
        """the sequence of checked values in the order the solver checks them: [(step, value / |b|, is the restart's true residual)]"""
        out = []
        for k in range(self.kmax + 1):
            if k in self.est:
                out.append((k, float(self.est[k] / self.bnorm), False))
            if k in self.true:
                out.append((k, float(self.true[k] / self.bnorm), True))
        return out


@functools.lru_cache(maxsize=None)
def reference(op, guess="zero"):
    """b = rhs(op.n); guess "zero" or "visible" (x_ref (1 + 0.5 xi), x_ref = iterate KMAX from zero)"""
    b = rhs(op.n)
    if guess == "zero":
        return Reference(op, b, np.zeros(op.n))
    x_ref = np.asarray(reference(op, "zero").xs[KMAX], dtype=np.float64)
    if guess == "visible":
        return Reference(op, b, x_ref * (1 + 0.5 * np.random.default_rng([SEED, op.n, 1]).standard_normal(op.n)))
    raise ValueError(guess)


REORTH_DELTA = 1e-10
REORTH_DIM = 5


def inverse_preconditioner(op, v):
    """P^-1 v = L D U' v, block by block from the factors (Ifpack's storage: unit lower L, 1 / d on the diagonal, U' = U / d), in
    extended precision"""
    _, diag, low, up = op._prepared(LD)
    x = np.asarray(v).astype(LD)
    y = x.copy()
    for i in range(op.n):
        c, val = up[i]
        if len(c):
            y[i] = x[i] + val @ x[c]
    y = y / diag
    z = y.copy()
    for i in range(op.n):
        c, val = low[i]
        if len(c):
            z[i] = y[i] + val @ y[c]
    return z


def nearly_invariant_rhs(op, delta=REORTH_DELTA):
    """b with P b = v0, v0 = the sum of an orthonormal basis of a real invariant subspace of M = P S of dimension 5 (eigenvalues spread
    over the spectrum) + delta x a unit vector outside it.  From x = 0 the Krylov space of the first five iterations is that subspace to
    delta: at inner == 4 the sweep leaves s / |vv| of the size of delta, and SolverGMRES re-orthogonalises from the fifth iteration on."""
    n = op.n
    S = np.zeros((n, n))
    S[np.repeat(np.arange(n), np.diff(op.rp)), op.ci] = op.sv
    w, V = np.linalg.eig(op.solve(S))                       # M, column by column
    real = [i for i in np.argsort(w.real) if w[i].imag == 0]
    assert len(real) >= REORTH_DIM
    pick = [real[int(j)] for j in np.linspace(0, len(real) - 1, REORTH_DIM)]
    Q, _ = np.linalg.qr(V[:, pick].real)
    out = np.random.default_rng([SEED, n, 5]).standard_normal(n)
    out -= Q @ (Q.T @ out)
    out /= np.linalg.norm(out)
    return np.asarray(inverse_preconditioner(op, Q @ np.ones(REORTH_DIM) + delta * out), dtype=np.float64)


REORTH_KMAX = 33


@functools.lru_cache(maxsize=None)
def reorth_reference(op):
    """the reference of the nearly invariant case from the zero guess; all three chains must take SolverGMRES' branch at step 5 with
    s / |vv| at least ten times under 10 sqrt(eps) and above 1e-12 (asserted here, on the CPU)"""
    ref = Reference(op, nearly_invariant_rhs(op), np.zeros(op.n), kmax=REORTH_KMAX)
    for c in [ref.ld] + ref.chains:
        assert c.reorth_from == REORTH_DIM and 1e-12 < c.ratio5 < 1.5e-8, (c.reorth_from, c.ratio5)
    return ref


@functools.lru_cache(maxsize=None)
def velocity_reference(op):
    """the velocity system from the zero guess, VELOCITY_KMAX steps (one restart)"""
    return Reference(op, rhs(op.n), np.zeros(op.n), kmax=VELOCITY_KMAX)


def bounds(ref, k):
    return K * (ref.err64_x[k] + FLOOR), K * (ref.err64_res[k] + FLOOR)


def iterates(ref, wanted=ITERATES):
    """the steps of `wanted` at which the reference alone keeps both bounds below HARD_LIMIT"""
    return tuple(k for k in wanted if k <= ref.kmax and max(bounds(ref, k)) < HARD_LIMIT)


def stops(ref):
    """[(rtol, step, at_restart)]: thresholds, relative to |b|, halfway (geometrically) between two record lows of the sequence of
    checked values, where both are further from the threshold than 10 x the residual bound of that step (in units of |b|); the step and
    the kind of check that meets the threshold first; and rtol = 1e-2 where every checked value stays 1 % clear of it"""
    seq = ref.checks()
    out, runmin = [], seq[0][1]
    scale = float(ref.pbnorm / ref.bnorm)
    for k, v, at_restart in seq[1:]:
        if v < 0.99 * runmin:
            thr = float(np.sqrt(runmin * v))
            bx, br = bounds(ref, k)
            if min(runmin - thr, thr - v) > 10 * br * scale and max(bx, br) < HARD_LIMIT:
                out.append((thr, k, at_restart))
        runmin = min(runmin, v)
    hit = [(k, r) for k, v, r in seq if v <= 1e-2]
    if hit and all(abs(v / 1e-2 - 1) >= 0.01 for _, v, _ in seq) and max(bounds(ref, hit[0][0])) < HARD_LIMIT:
        out.append((1e-2, hit[0][0], hit[0][1]))
    return out


def compare(ref, k, x, last, at_restart=False):
    """iterate and reported residual of a solve that ended at step k.  Returns (failures, ratios = error / (bound / K))"""
    x = np.asarray(x, dtype=np.float64)
    if x.shape != (ref.op.n,):
        return ["x has shape %s" % (x.shape,)], {}
    if not (np.all(np.isfinite(x)) and np.isfinite(last)):
        return ["x or the residual not finite"], {}
    if not 0 <= k <= ref.kmax:
        return ["%d steps: beyond the reference's %d" % (k, ref.kmax)], {}
    bx, br = bounds(ref, k)
    assert bx < HARD_LIMIT and br < HARD_LIMIT, (k, bx, br)   # the check itself: no bound may be this loose
    ex = float(np.max(np.abs(x - ref.xs[k])) / ref.scale[k])
    er = float(abs(LD(last) - ref.last(k, at_restart)) / ref.pbnorm)
    failures = []
    if not ex <= bx:
        failures.append("x_%d: error %.3e > bound %.3e (err64 %.3e)" % (k, ex, bx, ref.err64_x[k]))
    if not er <= br:
        failures.append("res_%d: error %.3e > bound %.3e (err64 %.3e)" % (k, er, br, ref.err64_res[k]))
    return failures, {"x": ex / (bx / K), "res": er / (br / K)}


def check_iterate(ref, k, out):
    """a call with tolerance 0 and maxiter = k from the reference's guess: status 1 after exactly k steps, x_k and the value checked
    last; k = 0 returns the guess bit for bit"""
    failures = []
    if out["status"] != 1 or out["steps"] != k:
        failures.append("status %d after %d steps, expected 1 after %d" % (out["status"], out["steps"], k))
    if k == 0 and not np.array_equal(np.asarray(out["x"], dtype=np.float64).view(np.uint64), ref.x0.view(np.uint64)):
        failures.append("maxiter = 0 changed x")
    f, ratios = compare(ref, k, out["x"], out["last_residual"])
    return failures + f, ratios


def check_stop(ref, steps_ref, at_restart, out):
    """a call with a tolerance: status 0 after EXACTLY the reference's steps, with that iterate and the value that met the tolerance"""
    failures = []
    if out["status"] != 0 or out["steps"] != steps_ref:
        failures.append("status %d after %d steps, expected 0 after %d" % (out["status"], out["steps"], steps_ref))
    if steps_ref == 0 and not np.array_equal(np.asarray(out["x"], dtype=np.float64).view(np.uint64), ref.x0.view(np.uint64)):
        failures.append("a solve that was converged at step 0 changed x")
    f, ratios = compare(ref, steps_ref, out["x"], out["last_residual"], at_restart)
    return failures + f, ratios


def as_out(s):
    """a Solve as Nsx.gmres returns it"""
    return {"x": np.asarray(s.x, dtype=np.float64), "steps": s.steps, "status": s.status, "last_residual": float(s.last)}
