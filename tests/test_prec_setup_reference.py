"""CPU suite of tests/prec_setup_reference.py, the reference and the bounds tests/test_gpu_prec_setup.py holds the preconditioner set-up
to.  Fed with the ORACLE's matrices the reference reproduces oracle.schur() inside the bound for the four preconditioner types on the
four meshes of the GPU suite -- the oracle exposes none of D, D_inv, lump_M, so the weights built from the reference's own float64
vectors giving the oracle's S inside the bound is their agreement -- every mutant leaves its bound or the exact-zero condition on the
mesh where it applies, and the meshes have the rows the GPU cases rely on."""
import numpy as np
import pytest

import prec_setup_reference as R
from conftest import Problem

MESHES = {"A": ("cylinder", 3, 1, {}), "B": ("cylinder", 2, 2, {}), "box3": ("box", 3, 1, {"n": [1, 1, 1]}), "box2": ("box", 2, 1, {"n": [1, 1]}),
          "B2": ("cylinder", 2, 2, {"n_sub": 2})}
_cases = {}


def boundary_values(p):
    if p.kind == "cylinder":
        from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
        return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2), p.deltat)
    bd = np.sort(p.dofs.boundary_dofs(0)).astype(np.int32)
    return bd, np.linspace(0.5, 1.5, len(bd))


def case(mesh):
    """(problem, oracle with boundary values applied, Setup on its matrices) of one mesh"""
    if mesh not in _cases:
        from navierstokes_project_nm4pde_amd import nsx
        kind, dim, level, kw = MESHES[mesh]
        p = Problem(kind, dim, level, **kw)
        ora = p.oracle()
        np.copyto(ora.solution, p.smooth_velocity())
        ora.assemble(nsx.TEMAM)
        bd, vals = boundary_values(p)
        ora.apply_boundary_values(bd, vals)
        _cases[mesh] = (p, ora, R.setup_from(p.dofs, ora.matrix, bd))
    return _cases[mesh]


def oracle_schur(ora, s, ptype):
    ora.prec_initialize(ptype)
    S = ora.schur()
    S.sort_indices()
    assert np.array_equal(S.indptr, s.terms.rp) and np.array_equal(S.indices, s.terms.ci), "the oracle's pattern is not that of B B^T"
    return S.data


@pytest.mark.parametrize("ptype", list(R.TYPES))
@pytest.mark.parametrize("mesh", ["A", "B", "box3", "box2"])
def test_reference_reproduces_the_oracle(mesh, ptype):
    p, ora, s = case(mesh)
    t = R.TYPES[ptype]
    v = oracle_schur(ora, s, t)
    w = R.weights64(s, t)
    ref = R.Schur(s, w["w"])
    msgs, ratio = R.compare_schur(ref, v)
    print("%s %s: oracle S error / bound = %.4f" % (mesh, ptype, ratio))
    assert not msgs, msgs
    assert 0 < ratio < 1
    # the float64 restatement, too, and its vectors: exact reciprocals, a lumped mass inside its bound, zeros where the mask says so
    assert not R.compare_schur(ref, R.schur64(s, w["w"]))[0]
    assert np.array_equal(w["D_inv"] * w["D"] > 0, np.ones(s.n_u, bool)) and np.array_equal(w["neg_D_inv"], -w["D_inv"])
    assert np.array_equal(w["D"][::s.dim], (s.mass if t == R.YOSIDA else s.F)[s.diag])
    if t == R.AYOSIDA:
        msgs, ratio = R.compare_lump(R.Lump(s), w["lump_M"])
        assert not msgs and ratio < 1, msgs
    assert np.all(w["w"][s.constrained] == 0.0) and np.count_nonzero(w["w"]) == s.n_u - len(s.constrained)
    zero = ref.A == 0
    assert np.all(v[zero] == 0.0) and np.all(ref.y[zero] == 0)
    # a stored entry that is not exactly 0 where every term is masked is reported, however small
    if np.any(zero):
        bad = v.copy()
        bad[np.nonzero(zero)[0][0]] = 1e-300
        assert "exactly 0 expected" in R.compare_schur(ref, bad)[0][0]


def test_meshes_have_the_rows_the_gpu_cases_rely_on():
    for mesh, (long_S, long_B, masked) in {"A": (49, 261, 4298), "B": (0, 0, 208)}.items():
        p, ora, s = case(mesh)
        ref = R.Schur(s, R.weights64(s, R.YOSIDA)["w"])
        nodes = np.array([len(np.unique(s.Bci[a:b] // s.dim)) for a, b in zip(s.Brp[:-1], s.Brp[1:])])
        assert (int(np.sum(np.diff(ref.rp) > 64)), int(np.sum(nodes > 64)), int(np.sum(ref.A == 0))) == (long_S, long_B, masked), mesh
        assert np.sum(s.mass < 0) > 0
    assert 3 * np.sum(case("A")[2].mass < 0) == 159396       # scalar entries x 3 components: an absolute row sum without fabs is another number
    for mesh, n in (("box3", 8), ("box2", 4)):
        s = case(mesh)[2]
        assert np.all(np.diff(s.terms.rp) == n) and s.n_p == n


@pytest.mark.parametrize("mutant,mesh,ptype", [("no_abs", "B", "ayosida"), ("mask_dropped", "B", "yosida"), ("last_common", "B", "yosida"),
                                               ("last_common", "box2", "simple"), ("one_component", "A", "yosida"), ("one_component", "B", "asimple"),
                                               ("tail_row", "A", "yosida"), ("ghost_weight", "B2", "yosida"), ("mask_dropped", "box3", "ayosida")])
def test_every_mutant_is_caught(mutant, mesh, ptype):
    p, ora, s = case(mesh)
    t = R.TYPES[ptype]
    good = R.weights64(s, t)
    ref = R.Schur(s, good["w"])
    assert not R.compare_schur(ref, R.schur64(s, good["w"]))[0]
    if mutant == "no_abs":
        msgs, ratio = R.compare_lump(R.Lump(s), R.weights64(s, t, mutant)["lump_M"])
        assert msgs and ratio > 1e6
        return
    if mutant == "mask_dropped":
        w = R.weights64(s, t, mutant)["w"]
        assert not np.array_equal(w, good["w"])                      # the weights' own bitwise comparison sees it ...
        msgs, ratio = R.compare_schur(ref, R.schur64(s, w), limit=10 ** 6)
        assert ratio > 1e6                                           # ... and so do the product's bound and, where a pair of rows
        assert np.any(ref.A == 0) == (mesh != "box3")                # shares constrained columns only (not on the 3D box), its zeros
        assert any("exactly 0 expected" in m for m in msgs) == (mesh != "box3")
        return
    kw = {}
    if mutant == "ghost_weight":
        assert p.dofs.n_subdomains == 2
        kw = {"u_ptr": p.dofs.owned_u_ptr, "p_ptr": p.dofs.owned_p_ptr}
    if mutant == "tail_row":
        kw = {"prev": R.schur64(s, R.weights64(s, R.SIMPLE)["w"])}   # the values an earlier initialisation of another type left
    msgs, ratio = R.compare_schur(ref, R.schur64(s, good["w"], mutant, **kw))
    print("%s on %s: error / bound = %.3g" % (mutant, mesh, ratio))
    assert msgs and ratio > 1e3
