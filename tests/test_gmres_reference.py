"""CPU suite: the extended-precision reference of the GMRES driver tests (tests/gmres_reference.py) is right, and its comparisons bite:
deliberately wrong restatements of SolverGMRES -- the ways gmres() in csrc/nsx_solve.hip can be subtly wrong while a converged solve
still looks fine -- FAIL them, with the margin K the GPU module (tests/test_gpu_gmres.py) asserts with.  The data are the oracle's
Schur complement and factors on the GPU module's meshes (3D level-1 cylinder, 745 rows; 2D level-2 cylinder, 366 rows; 96-row blocks).

Mutants (gmres_reference.MUTANTS) and the call that shows each:
  givens_sign               gamma_{k+1} = +s gamma_k: iterates from step 2 on (the size of the estimate does not change: only x does)
  x0_ignored                the first update stores the sum alone: every iterate from a guess that is not zero
  second_cycle_overwrites   x = sum in the second cycle: iterates beyond step 28
  tol_b_squared             the tolerance rtol |b|^2: the step count at a relative tolerance
h2_omitted, norm_of_first_sweep and no_restart_residual are NOT rejected, on any input tried: see
test_what_the_second_sweep_changes_is_of_rounding_size, which measures them on the nearly invariant case where the second sweeps run."""
import numpy as np
import pytest

import gmres_reference as G
from test_cg_reference import operator

NAMES = ["A96", "B96"]


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_gmres(name):
    """left-preconditioned GMRES: the estimate equals the true preconditioned residual of the iterate, at every kept step, and the
    checked values never grow inside a cycle"""
    op = operator(name)
    ref = G.reference(op, "zero")
    assert ref.xs[0].dtype == np.longdouble and ref.kmax == G.KMAX and ref.reorth_from is None
    for k in (1, 13, 28, 29, 57):
        r = op.solve(ref.b.astype(G.LD) - op.apply(ref.xs[k], G.LD), G.LD)
        assert float(abs(np.sqrt(np.sum(r * r)) - ref.est[k]) / ref.pbnorm) < 1e-15, k
    assert sorted(ref.true) == [0, 28, 56]
    assert float(abs(ref.true[28] - ref.est[28]) / ref.pbnorm) < 1e-15
    seq = [v for _, v, _ in ref.checks()]
    assert all(b <= a * (1 + 1e-12) for a, b in zip(seq, seq[1:]))


@pytest.mark.parametrize("guess", ["zero", "visible"])
@pytest.mark.parametrize("name", NAMES)
def test_float64_chains_pass_and_every_iterate_is_kept(name, guess):
    ref = G.reference(operator(name), guess)
    assert G.iterates(ref) == G.ITERATES                 # nothing had to be dropped: every bound stays below HARD_LIMIT
    assert max(G.bounds(ref, G.KMAX)) < 0.5 * G.HARD_LIMIT
    stops = G.stops(ref)
    assert len(stops) >= 20 and any(k > G.RESTART for _, k, _ in stops)
    for c in ref.chains:
        for k in G.ITERATES:
            out = {"x": np.asarray(c.xs[k], dtype=np.float64), "steps": k, "status": 1, "last_residual": float(c.true[0] if k == 0 else c.est[k])}
            fails, ratios = G.check_iterate(ref, k, out)
            assert not fails and max(ratios.values()) <= 1.0 + 1e-9, (k, fails, ratios)
    for dots, precond in (("pairwise", "tri"), ("sequential", "dense")):
        for rtol, k, at_restart in stops[::7]:
            s = G.gmres(ref.op, ref.x0, ref.b, 0.0, 100000, np.float64, dots, precond, rtol=rtol)
            fails, _ = G.check_stop(ref, k, at_restart, G.as_out(s))
            assert not fails, (rtol, k, fails)


def _iterate_fails(ref, k, **kw):
    s = G.gmres(ref.op, ref.x0, ref.b, 0.0, k, np.float64, **kw)
    fails, _ = G.check_iterate(ref, k, G.as_out(s))
    return fails


@pytest.mark.parametrize("name", NAMES)
def test_wrong_restatements_fail_the_comparisons(name):
    op = operator(name)
    zero, visible = G.reference(op, "zero"), G.reference(op, "visible")
    for ref in (zero, visible):
        for k in (29, 33, 56, 57):
            assert not _iterate_fails(ref, k)
            assert _iterate_fails(ref, k, mutant="second_cycle_overwrites"), k
        for k in (2, 3, 13, 28, 57):
            assert _iterate_fails(ref, k, mutant="givens_sign"), k
        for k in (1, 13, 28):                                # inside the first cycle it is not wrong
            assert not _iterate_fails(ref, k, mutant="second_cycle_overwrites")
    for k in (1, 2, 13, 28, 33):
        assert _iterate_fails(visible, k, mutant="x0_ignored"), k
        assert not _iterate_fails(zero, k, mutant="x0_ignored")                 # (from a zero guess there is nothing to ignore)
    for ref in (zero, visible):
        hit = 0
        for rtol, k, at_restart in G.stops(ref)[::5]:
            s = G.gmres(op, ref.x0, ref.b, 0.0, 100000, np.float64, rtol=rtol, mutant="tol_b_squared")
            hit += bool(G.check_stop(ref, k, at_restart, G.as_out(s))[0])
        assert hit >= 3


def test_nearly_invariant_case_takes_the_re_orthogonalising_branch():
    """the case tests/test_gpu_gmres.py runs for SolverGMRES' second sweeps (366-row Schur system): P b lies in a 5-dimensional invariant
    subspace of P S up to delta = 1e-10, so that at the fifth iteration s / |vv| = 5.2e-9 in all three chains -- more than ten times
    under 10 sqrt(eps) = 1.5e-7, above 1e-12 (asserted by reorth_reference) -- and every later iteration sweeps twice.  The bounds stay
    below HARD_LIMIT through step 33 and the float64 chains pass, in iterates and in stopping steps behind the fifth iteration."""
    op = operator("B96")
    ref = G.reorth_reference(op)
    assert ref.reorth_from == 5 and 1e-9 < ref.ld.ratio5 < 1.5e-8
    assert float(ref.est[5] / ref.est[4]) < 1e-8          # the residual collapses when the subspace is exhausted
    for k in (4, 5, 6, 8, 13, 29, 33):
        assert max(G.bounds(ref, k)) < G.HARD_LIMIT
        assert not _iterate_fails(ref, k)
        assert _iterate_fails(ref, k, mutant="givens_sign")
    stops = [s for s in G.stops(ref) if 6 <= s[1] <= 11]
    assert len(stops) >= 3
    for rtol, k, at_restart in stops:
        s = G.gmres(op, ref.x0, ref.b, 0.0, 200, np.float64, "sequential", "dense", rtol=rtol)
        assert s.reorth_from == 5 and not G.check_stop(ref, k, at_restart, G.as_out(s))[0]


def test_what_the_second_sweep_changes_is_of_rounding_size():
    """WHY h2_omitted, norm_of_first_sweep and no_restart_residual are not among the mutants the comparison rejects, measured on the
    nearly invariant case where the second sweeps really run: after a first sweep that leaves s / |vv| = 5e-9 the vector has lost
    orthogonality by eps / 5e-9 = 4e-8 of ITS OWN length s, so the second sweep's coefficients are 4e-8 s = 2e-16 |vv| -- an ulp of the
    Hessenberg column they are added to -- and its norm differs from the first sweep's by (4e-8)^2.  A left-preconditioned GMRES'
    estimate IS the true preconditioned residual in exact arithmetic, so carrying it over a restart changes nothing beyond rounding
    either.  The three wrong solves stay inside a THIRD of the bound (asserted: if a future input makes one of them visible, this test
    says so and the mutant belongs with the rejected ones).  What the comparison on the device can show of that branch is that it ran
    (the second sweeps in the profile table) and that the iterates behind it are right."""
    op = operator("B96")
    ref = G.reorth_reference(op)
    for mutant in ("h2_omitted", "norm_of_first_sweep", "no_restart_residual"):
        for k in (5, 8, 13, 29, 33):
            s = G.gmres(op, ref.x0, ref.b, 0.0, k, np.float64, mutant=mutant)
            assert s.reorth_from == 5
            fails, ratios = G.check_iterate(ref, k, G.as_out(s))
            assert not fails and max(ratios.values()) <= G.K / 3, (mutant, k, ratios)


def test_velocity_reference_on_the_weak_preconditioner():
    """F and its block-Jacobi ILU(0) over 8 subdomains of the 3D level-1 cylinder (the oracle's data): every iterate of
    VELOCITY_ITERATES is kept (err64 5e-15 through the restart), the float64 chains pass, wrong solves do not"""
    import oracle
    import sparse_reference as SR
    from conftest import Problem
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    p = Problem("cylinder", 3, 1, n_sub=8, ordering="colour")
    o = p.oracle()
    o.solution[:] = p.smooth_velocity()
    o.assemble(1)
    o.apply_boundary_values(*cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2), p.deltat))
    o.prec_initialize(oracle.YOSIDA)
    sel, graph = SR.scalar_selection(p.dofs)
    op = G.VelocityOperator(graph[0], graph[1], np.array(o.matrix(0, 0))[sel], np.array(o.ilu_F())[sel], p.dofs.owned_u_ptr, p.dim)
    ref = G.velocity_reference(op)
    assert G.iterates(ref, G.VELOCITY_ITERATES) == G.VELOCITY_ITERATES and ref.err64_x[33] < 1e-13
    for k in (5, 13, 28, 29, 33):
        assert not _iterate_fails(ref, k) and not _iterate_fails(ref, k, dots="sequential")
        assert _iterate_fails(ref, k, mutant="givens_sign"), k
    for k in (29, 33):
        assert _iterate_fails(ref, k, mutant="second_cycle_overwrites"), k
