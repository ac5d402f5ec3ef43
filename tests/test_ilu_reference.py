"""CPU suite: the extended-precision reference of the ILU(0) tests (tests/ilu_reference.py) is right, and its comparisons bite.
On the oracle's matrices -- the scalar F after apply_boundary_values and negative_S_tilde, on the 2D level-2 and the 3D level-1
cylinder (the GPU module's meshes) -- it shows that
  * in long double (L D U)_ij = a_ij on the in-block pattern to a few long-double eps of s_ij: ILU(0)'s defining property;
  * the float64 restatements agree with the oracle's factors and with oracle.ilu0_solve within the yardstick;
  * the reference solve agrees with the host replay of the lane-owner stream for 1..4 entries per tick, with and without float values;
  * every deliberately wrong variant exceeds the asserted bound at least 100 times."""
import numpy as np
import pytest

import ilu_reference as R
from conftest import Problem

MESHES = {"A": (3, 1), "B": (2, 2)}
# blocks of F (P2 nodes) and of S per configuration; "one" = the whole matrix as a single block
LAYOUTS = {"one": lambda n: R.block_ptr(n, n), "85": lambda n: R.block_ptr(n, 85), "96": lambda n: R.block_ptr(n, 96)}
CONFIGS = [("A", "one"), ("A", "85"), ("B", "one"), ("B", "85")]
_data = {}


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2), time)


def data(mesh, layout):
    """{which: (rp, ci, values, block pointer, the oracle's factors)} of a Yosida initialisation, which = "F" / "S" """
    if (mesh, layout) not in _data:
        import oracle
        dim, level = MESHES[mesh]
        p = Problem("cylinder", dim, level)
        o = p.oracle()
        n2 = p.dofs.n_u // dim
        fptr = LAYOUTS[layout](n2)
        sptr = LAYOUTS["96" if layout == "85" else layout](p.dofs.n_p)
        if layout != "one":
            pp = np.round(fptr.astype(np.float64) * p.dofs.n_p / n2).astype(np.int32)
            o.set_ranks(fptr, pp)
            o.set_schur_blocks(sptr)
        o.solution[:] = p.smooth_velocity()
        o.assemble(1)
        o.apply_boundary_values(*_bc(p, p.deltat))
        o.prec_initialize(oracle.YOSIDA)
        g0 = o.graphs[0]
        rows = np.repeat(np.arange(len(g0[0]) - 1), np.diff(g0[0]))
        sel = (rows % dim == 0) & (g0[1] % dim == 0)     # same-component entries carry the scalar F
        rp = np.zeros(n2 + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows[sel] // dim, minlength=n2), out=rp[1:])
        S = o.schur()
        _data[(mesh, layout)] = {"F": (rp, g0[1][sel] // dim, o.matrix(0, 0)[sel].copy(), fptr, o.ilu_F()[sel], dim),
                                 "S": (S.indptr, S.indices, S.data, sptr, o.ilu_S(S.nnz), 1)}
    return _data[(mesh, layout)]


_refs = {}


def factor_ref(mesh, layout, which):
    key = (mesh, layout, which)
    if key not in _refs:
        rp, ci, a, ptr, _, _ = data(mesh, layout)[which]
        _refs[key] = R.FactorReference(rp, ci, a, ptr)
    return _refs[key]


@pytest.mark.parametrize("which", ["F", "S"])
@pytest.mark.parametrize("mesh,layout", CONFIGS)
def test_long_double_factors_reproduce_the_matrix_on_the_pattern(mesh, layout, which):
    """(L D U)_ij = a_ij for every in-block entry: sum_{k < min(i,j)} l_ik u_kj + (l_ij d_j | d_i | u_ij), from the STORED factors"""
    ref = factor_ref(mesh, layout, which)
    g, lu = ref.g, ref.lu
    d = 1 / lu[g.diag]
    worst = 0.0
    for r0, r1 in R._blocks(g.bptr):
        nb = r1 - r0
        Urow = {}
        for i in range(r0, r1):                          # U_i. = d_i * (U/d)_i. , diagonal included
            c = g.ci[g.diag[i]:g.hi[i]] - r0
            v = lu[g.diag[i]:g.hi[i]] * d[i]
            v[0] = d[i]
            Urow[i] = (c, v)
        acc, sacc = np.zeros(nb, dtype=R.LD), np.zeros(nb, dtype=R.LD)
        for i in range(r0, r1):
            lo, hi, dg = g.lo[i], g.hi[i], g.diag[i]
            cols = g.ci[lo:hi] - r0
            acc[:] = 0
            sacc[:] = 0
            for p in list(range(lo, dg)) + [None]:
                k, l = (g.ci[p], lu[p]) if p is not None else (i, R.LD(1))
                c, v = Urow[k]
                acc[c] += l * v
                sacc[c] += np.abs(l * v)
            den = sacc[cols] + np.abs(ref.a[lo:hi])
            err = np.abs(acc[cols] - ref.a[lo:hi]) / np.where(den > 0, den, np.finfo(np.float64).tiny)
            worst = max(worst, float(np.max(err)))
    assert worst <= 8 * float(np.finfo(R.LD).eps), worst


@pytest.mark.parametrize("which", ["F", "S"])
@pytest.mark.parametrize("mesh,layout", CONFIGS)
def test_float64_restatements_agree_with_the_oracle_within_the_yardstick(mesh, layout, which):
    import oracle
    rp, ci, a, ptr, lu_oracle, ncomp = data(mesh, layout)[which]
    ref = factor_ref(mesh, layout, which)
    # the yardstick is of rounding size: 2 - 10 eps, the 2D Schur matrix as ONE block 2e-13 (366 rows coupled through one elimination)
    assert ref.err64 <= (1e-12 if (mesh, layout, which) == ("B", "one", "S") else 64 * R.EPS), ref.err64
    assert ref.bound(max(R.K_FACTOR, 10.0)) < R.HARD_LIMIT
    for form, lu in ref.forms.items():
        f, ratio = R.compare_factor(ref, lu, k_margin=2.0)
        assert not f and ratio <= 1.0, (form, f)
    f, ratio = R.compare_factor(ref, lu_oracle, k_margin=2.0)       # the oracle is one more float64 restatement of the sweep
    assert not f, f
    assert np.all(ref.lu[~ref.inside] == 0) and np.all(lu_oracle[~ref.inside] == 0)
    # solves on the oracle's factors: sweeps, explicit inverses and oracle.ilu0_solve against the long-double solve
    b = R.rhs(ref.g.n, ncomp)
    sref = R.SolveReference(ref.g, lu_oracle, b, ncomp)
    assert sref.err64 <= 256 * R.EPS, sref.err64
    x = np.empty_like(b)
    for c in range(ncomp):
        x[c::ncomp] = oracle.ilu0_solve(rp, ci, lu_oracle, ptr, b[c::ncomp])
    f, ratio = R.compare_solve(sref, x, k_margin=2.0)
    assert not f, f
    assert not np.any(R.solve(rp, ci, lu_oracle, ptr, np.zeros_like(b), ncomp, np.float64, graph=ref.g))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("mesh,which", [("B", "F"), ("B", "S"), ("A", "S")])
def test_reference_solve_agrees_with_the_host_replay_of_the_stream(mesh, which, f32):
    from navierstokes_project_nm4pde_amd.frontend import ilu_stream_apply
    rp, ci, a, ptr, lu, ncomp = data(mesh, "85")[which]
    ref = factor_ref(mesh, "85", which)
    b = R.rhs(ref.g.n, ncomp)
    sref = R.SolveReference(ref.g, lu, b, ncomp, stream_float=f32)
    assert sref.err64 <= 256 * R.EPS
    for ept in (1, 2, 3, 4):
        x = ilu_stream_apply(rp, ci, ptr, lu, b, ncomp, 3, 2, ept, f32=f32)
        f, ratio = R.compare_solve(sref, x, k_margin=2.0)       # the replay is the sweep with fused multiply-adds: another float64 grouping
        assert not f, (ept, f)
    if f32:                                                       # ... and the float stream is visible: the double solve does not pass for it
        f, _ = R.compare_solve(sref, R.solve(rp, ci, lu, ptr, b, ncomp, np.float64, graph=ref.g))
        assert f


def _mutation_rows(ref):
    """rows where a wrong variant shows.  (1) For the skipped update: the row whose skipped term -- the FIRST pivot row's last in-block
    entry that has a partner in the row -- is the largest against the partner's absolute-term sum (rows of Dirichlet nodes are unit
    rows: nothing is ever subtracted from them).  (2) A row in the middle of the first block of at least 32 rows that has in-block
    entries in front of its diagonal and non-zero ones behind it, and a pivot other than 1."""
    g, lu, s = ref.g, ref.lu, ref.s
    d = 1 / lu[g.diag]
    best, best_row = 0.0, None
    for i in range(g.n):
        lo, hi, dg = g.lo[i], g.hi[i], g.diag[i]
        for p in range(lo, dg):
            k = g.ci[p]
            if g.hi[k] > g.diag[k] + 1:
                q = lo + np.searchsorted(g.ci[lo:hi], g.ci[g.hi[k] - 1])
                if q < hi and g.ci[q] == g.ci[g.hi[k] - 1]:
                    term = abs(lu[p] * d[k] * lu[g.hi[k] - 1])                      # |a_ik (U_kj / d_k)|
                    raw = s[q] * (abs(d[g.ci[q]]) if q < dg else d[i] * d[i] if q == dg else abs(d[i]))   # s_ij before the storage transform
                    if raw > 0 and term / raw > best:
                        best, best_row = float(term / raw), i
                    break
    assert best > 0.01, best
    r0, r1 = next((a, b) for a, b in R._blocks(g.bptr) if b - a >= 32)
    mid = next(i for i in range((r0 + r1) // 2, r1) if g.diag[i] > g.lo[i] and abs(d[i] - 1) > 0.01
               and np.max(np.abs(lu[g.diag[i] + 1:g.hi[i]]), initial=0) > 1e-3)   # (couplings to Dirichlet columns are zeros: nothing to scale)
    return best_row, mid


@pytest.mark.parametrize("which", ["F", "S"])
@pytest.mark.parametrize("mesh", ["A", "B"])
def test_wrong_factorisations_exceed_the_bound_by_a_clear_factor(mesh, which):
    rp, ci, a, ptr, _, _ = data(mesh, "85")[which]
    ref = factor_ref(mesh, "85", which)
    last, mid = _mutation_rows(ref)
    bound = ref.bound()
    wrong = {"one update of a pivot row's last in-block entry skipped": dict(skip_update=last),
             "the strongest coupling to an earlier block kept": dict(cross_block=True),
             "a row's upper triangle left unscaled": dict(unscaled_upper=mid)}
    for what, kw in wrong.items():
        lu, _ = R.factor(rp, ci, a, ptr, np.float64, graph=ref.g, **kw)
        f, _ = R.compare_factor(ref, lu)
        assert f, what
        assert ref.error(lu) >= 100 * bound, (what, ref.error(lu), bound)


@pytest.mark.parametrize("which", ["F", "S"])
@pytest.mark.parametrize("mesh", ["A", "B"])
def test_wrong_solves_exceed_the_bound_by_a_clear_factor(mesh, which):
    rp, ci, a, ptr, lu, ncomp = data(mesh, "85")[which]
    ref = factor_ref(mesh, "85", which)
    g = ref.g
    b = R.rhs(g.n, ncomp)
    sref = R.SolveReference(g, lu, b, ncomp)
    _, mid = _mutation_rows(ref)
    p = g.cross_entry(a)
    cross = (int(g.rows[p]), int(g.ci[p]), a[p] * lu[g.diag[g.ci[p]]])
    for what, kw in {"the D^-1 scaling of one row skipped": dict(skip_dinv=mid), "a coupling across a block boundary kept": dict(cross_block=cross)}.items():
        x = R.solve(rp, ci, lu, ptr, b, ncomp, np.float64, graph=g, **kw)
        f, _ = R.compare_solve(sref, x)
        assert f, what
        assert sref.error(x) >= 100 * sref.bound(), (what, sref.error(x), sref.bound())


@pytest.mark.parametrize("mesh,which,ncomp,size", [("B", 0, 2, 85), ("A", 0, 3, 85), ("A", 1, 1, 96)])
def test_ragged_layouts_reach_every_exit_of_the_streams_sweep_loop(mesh, which, ncomp, size):
    """what the GPU module's stream matrix relies on (it checks the same on the device's own graphs before it runs): with one block per
    wave the ragged layout's sweeps have slab counts = 0, 4, 8 and 12 (mod 16) -- the four exits of the sweep loop in
    csrc/nsx_ilu_lanes.hpp -- and empty sweeps, for every number of entries per tick"""
    from navierstokes_project_nm4pde_amd.frontend import ilu_stream_stats
    from test_ilu_stream import scalar_graph
    dim, level = MESHES[mesh]
    rp, ci = scalar_graph(Problem("cylinder", dim, level).dofs, which)
    ptr = R.ragged_ptr(len(rp) - 1, size)
    assert ptr[0] == ptr[1] and ptr[-1] == ptr[-2] and np.any(np.diff(ptr)[1:-1] == 0)      # empty blocks in front, inside, at the end
    for ept in (1, 2, 3, 4):
        st = ilu_stream_stats(rp, ci, ptr, 1, ncomp, 2, ept)
        counts = st["fwd_slabs"] + st["bwd_slabs"]
        assert len(counts) == 2 * st["waves"] and sum(counts) == st["slabs"] and max(counts) <= st["max_wave_slabs"]
        assert {"empty" if c == 0 else c % 16 for c in counts} == {0, 4, 8, 12, "empty"}, (ept, sorted(set(counts)))
