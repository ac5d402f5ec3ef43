"""CPU suite: the extended-precision reference of the Schur CG tests (tests/cg_reference.py) is right, and its comparisons bite:
deliberately wrong restatements of SolverCG -- the ways a kernel of csrc/nsx_cg.hip can be subtly wrong while a converged solve still
looks fine -- FAIL them, with the margin K the GPU module (tests/test_gpu_schur_cg.py) asserts with.  The data are the oracle's Schur
complement and factors on the GPU module's smallest meshes and block layouts."""
import numpy as np
import pytest

import cg_reference as R
from conftest import Problem

# (mesh, block layout): uniform blocks of 96 / 256 rows and the ragged layout on the 3D level-1 cylinder, 96 on the 2D level-2 cylinder
CONFIGS = {"A96": ((3, 1), lambda n: R.block_ptr(n, 96)), "A256": ((3, 1), lambda n: R.block_ptr(n, 256)),
           "Aragged": ((3, 1), R.ragged_ptr), "B96": ((2, 2), lambda n: R.block_ptr(n, 96))}
_ops = {}


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2), time)


def operator(name):
    """the oracle's negative_S_tilde and ILU(0) factors of a Yosida initialisation, as an R.Operator (one per configuration)"""
    if name not in _ops:
        import oracle
        (dim, level), ptr_of = CONFIGS[name]
        p = Problem("cylinder", dim, level)
        o = p.oracle()
        ptr = ptr_of(p.dofs.n_p)
        o.set_schur_blocks(ptr)
        o.solution[:] = p.smooth_velocity()
        o.assemble(1)
        o.apply_boundary_values(*_bc(p, p.deltat))
        o.prec_initialize(oracle.YOSIDA)
        S = o.schur()
        _ops[name] = R.Operator(S.indptr, S.indices, S.data, o.ilu_S(S.nnz), ptr)
    return _ops[name]


@pytest.mark.parametrize("name", ["A96", "Aragged", "B96"])
def test_triangular_solve_equals_the_oracles(name):
    import oracle
    op = operator(name)
    g = np.random.default_rng(3).standard_normal(op.n)
    want = oracle.ilu0_solve(op.rp, op.ci, op.lu, op.bptr, g)
    got = op.solve(g)
    assert np.max(np.abs(got - want)) <= 64 * R.EPS * np.max(np.abs(want))     # the same operations, the sums in another order
    # ... the explicit inverses apply the same operator, and the extended-precision solve agrees with both to float64 rounding
    assert np.max(np.abs(op.dense(g) - want)) <= 1e-12 * np.max(np.abs(want))
    assert float(np.max(np.abs(op.solve(g, R.LD) - want))) <= 1e-12 * np.max(np.abs(want))


def test_reference_solves_the_system_in_extended_precision():
    """the chain is CG: the iterates converge to the solution of S x = b and the recursive residual is the true one to extended precision"""
    op = operator("A96")
    ref = R.reference(op, "zero")
    assert ref.xs[0].dtype == np.longdouble
    for k in (1, 10, R.KMAX):
        true = op.apply(ref.xs[k], R.LD) - ref.b.astype(R.LD)
        assert float(np.sqrt(np.sum(true * true)) / ref.bnorm) == pytest.approx(float(ref.res[k] / ref.bnorm), abs=1e-17)
    r = ref.rel_res()
    assert r[0] == pytest.approx(1.0) and r[R.KMAX] < 1e-2 < r[5]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_yardstick_is_of_rounding_size_and_the_inputs_do_their_job(name):
    op = operator(name)
    zero, visible, exact = (R.reference(op, g) for g in R.GUESSES)
    for ref in (zero, visible):
        # a few eps after 30 iterations on the 3D mesh; the 2D mesh (deltat = 1e-2) loses a digit more: 3.5e-14 / 2.0e-14 measured
        lim = 1e-14 if name.startswith("A") else 1e-13
        assert ref.err64_x[30] <= lim and ref.err64_res[30] <= lim, (ref.err64_x[30], ref.err64_res[30])
        assert max(R.bounds(ref, R.STOP_KMAX)) < R.HARD_LIMIT and max(R.bounds(ref, R.STOP_KMAX, R.K_DIST)) < R.HARD_LIMIT
        assert len(R.stops(ref)) >= 5
        assert (1e-2, int(np.flatnonzero(ref.rel_res() <= 1e-2)[0])) in R.stops(ref)  # the reference's own tolerance is among them
    # the visible guess leaves a trace: its residual history is another one from the first entry on
    assert abs(visible.rel_res()[0] - 1.0) > 0.1
    # the exact guess is converged at step 0 for rtol = 1e-2, with room
    assert exact.rel_res()[0] < 0.5e-2


@pytest.mark.parametrize("name", list(CONFIGS))
def test_float64_chains_pass_the_comparisons(name):
    """a correct float64 implementation passes with K = 2 already (ratios <= 1 by construction): nothing right is refused"""
    op = operator(name)
    refs = {g: R.reference(op, g) for g in R.GUESSES}
    for precond in ("tri", "dense"):
        failures, worst = run_schedule(op, refs, k_margin=2.0, precond=precond)
        assert not failures, failures
        assert worst <= 1.0
    assert not R.check_zero_rhs(R.cg(op, np.zeros(op.n), np.zeros(op.n), 1e-2, 100000, np.float64).out())


def run_schedule(op, refs, k_margin=None, precond="tri", first_failure_only=False, **wrong):
    """every call the GPU module makes for one configuration, answered by the float64 chain (restated wrongly by **wrong).  The calls
    with rtol = 0, maxiter = k are answered from ONE run with a history (iterate k does not depend on maxiter, in any of the
    restatements); the calls with a tolerance are solves of their own (a wrong one may never stop: at most KMAX + 5 iterations).  With
    the triangular solves (a Python loop over the rows) every fourth threshold and the reference's own rtol are run."""
    failures, worst = [], 0.0
    b = R.rhs(op.n)
    with np.errstate(all="ignore"):
        hist = {g: R.cg(op, refs[g].x0, b, 0.0, max(R.ITERATES), np.float64, precond, history=True, **wrong) for g in ("zero", "visible")}
        calls = R.schedule(refs["zero"], refs["visible"], refs["exact"])
        if precond == "tri":
            stop_calls = [c for c in calls if c[0] == "stop"]
            calls = [c for c in calls if c[0] != "stop"] + stop_calls[::4] + [c for c in stop_calls if c[2] == 1e-2]
        for kind, guess, rtol, maxiter, steps in calls:
            ref = refs[guess]
            if kind == "iterate":
                h = hist[guess]
                k = min(maxiter, len(h.xs) - 1)
                out = (np.asarray(h.xs[k], dtype=np.float64), k, float(h.res[k]), 1)
                f, ratios = R.check_iterate(ref, maxiter, out, k_margin)
            else:
                out = R.cg(op, ref.x0, b, rtol, R.KMAX + 5, np.float64, precond, **wrong).out()
                f, ratios = R.check_stop(ref, rtol, steps, out, k_margin)
            failures += ["%s %s rtol=%g maxiter=%d: %s" % (kind, guess, rtol, maxiter, m) for m in f]
            worst = max([worst] + list(ratios.values()))
            if failures and first_failure_only:
                break
    return failures, worst


MUTATIONS = {
    "beta from g.g": dict(beta_gg=True),
    "alpha with the g.h of the iteration before": dict(stale_gh=True),
    "d = beta d + h": dict(plus_h=True),
    "tolerance from |g_0|": dict(tol_g0=True),
    "stop test on sqrt(g.h)": dict(stop_gh=True),
    "one more update of x after the converging iteration": dict(extra_update=True),
    "last entry of the last block's last row left out of A d": dict(drop_tail=-1),
    "last entry of a block's last row left out of A d": dict(drop_tail="block_tail"),
    "a coupling across a block boundary kept in P": dict(cross_block=True),
    "a row's h left at its previous value": dict(stale_h="block_tail"),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_wrong_restatements_fail_the_comparisons(name, what):
    op = operator(name)
    refs = {g: R.reference(op, g) for g in R.GUESSES}
    wrong = dict(MUTATIONS[what])
    # (the graph of the product B D^-1 B^T has structural zeros, 1e-35 in value: a row whose last entry is one of them proves nothing)
    tails = [int(r) - 1 for r in op.bptr[1:] if abs(op.sv[op.rp[r] - 1]) > 1e-3 * np.max(np.abs(op.sv))]
    for key, v in wrong.items():
        if v == "block_tail":
            wrong[key] = tails[0]                 # the last row of the first block whose last entry is a real one
        elif v == -1:
            wrong[key] = tails[-1]
    failures, _ = run_schedule(op, refs, precond="tri" if "cross_block" in wrong else "dense", first_failure_only=True, **wrong)
    assert failures, "%s passed every comparison on %s" % (what, name)
    # ... and each wrong solve would still CONVERGE to the same solution (what the converged-solve tests see), except the ones
    # that change the operator or the preconditioner's symmetry
    if what in ("tolerance from |g_0|", "stop test on sqrt(g.h)", "one more update of x after the converging iteration"):
        ref = refs["visible"]
        good = R.cg(op, ref.x0, R.rhs(op.n), 1e-10, 2000, np.float64)
        bad = R.cg(op, ref.x0, R.rhs(op.n), 1e-10, 2000, np.float64, **wrong)
        assert good.status == 0 and bad.status == 0 and abs(good.steps - bad.steps) <= 8
        assert np.max(np.abs(good.x - bad.x)) <= 1e-8 * np.max(np.abs(good.x))
