"""CPU suite of tests/sparse_reference.py, the reference and the bound tests/test_gpu_sparse.py holds every sparse product kernel to:
correct float64 restatements in three summation orders stay inside the bound on the matrices of the 3D box mesh, four deliberately
wrong products leave it (the bound notices a subtly wrong kernel), and the host restatement of the chunk table of the LDS-staged kernel
cuts the crafted rank tables where the GPU cases expect it."""
import numpy as np
import pytest

import sparse_reference as R
from conftest import Problem

ORDERS = ("forward", "reversed", "lanes16")
NO_S = [op for op in R.OPS if op != "S"]            # the Schur complement is the device's own product: GPU suite only


@pytest.fixture(scope="module")
def box():
    """F, mass, B, G of the 3D box mesh (245 P2 rows of 8 - 65 entries), assembled by the oracle with boundary values applied"""
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("box", 3)
    ora = p.oracle()
    np.copyto(ora.solution, p.smooth_velocity())
    ora.assemble(nsx.TEMAM)
    bd = np.sort(p.dofs.boundary_dofs(0)).astype(np.int32)            # the face x = 0: every component of its 35 P2 nodes
    assert len(bd) == 105
    ora.apply_boundary_values(bd, np.linspace(0.5, 1.5, len(bd)))
    o = R.operators_from(p.dofs, ora.matrix)
    x, aux = R.vectors(o.n_u + o.n_p)
    return o, x, aux


def test_operators_are_what_the_suite_is_about(box):
    o, x, aux = box
    assert o.dim == 3 and o.n2 == 245 and np.max(np.diff(o.rp)) > 64 and np.min(np.diff(o.rp)) >= 1       # rows beyond 4 x 16 entries: the lanes wrap
    assert np.any(o.F != 0) and np.any(o.mass != 0) and np.any(o.B[2] != 0) and np.any(o.G[2] != 0)
    assert not np.array_equal(o.F, o.with_float_F().F) and np.array_equal(o.mass, o.with_float_F().mass)


@pytest.mark.parametrize("op", NO_S)
def test_correct_restatements_stay_inside_the_bound(box, op):
    o, x, aux = box
    ref = R.reference(o, op, x, aux)
    results = {order: R.product64(o, op, x, aux, order) for order in ORDERS}
    for order, y in results.items():
        msgs, ratio = R.compare(ref, y)
        print("%s %s: error / bound = %.4f" % (op, order, ratio))
        assert not msgs, (order, msgs)
        assert 0 < ratio < 1
    if op in ("F", "SADDLE"):                         # the orders do differ: the bound is not met by construction
        assert any(not np.array_equal(results["forward"], results[k]) for k in ("reversed", "lanes16"))
    # entries the op does not produce are exactly 0 in the reference and carry no allowance
    lo, hi = (o.n_u, o.n_u + o.n_p) if op in R.U_OPS else (0, o.n_u) if op in R.P_OPS else (0, 0)
    assert not np.any(ref.y[lo:hi]) and not np.any(ref.bound()[lo:hi])
    bad = results["forward"].copy()
    if hi > lo:
        bad[lo] = 1e-300
        assert R.compare(ref, bad)[0]


def test_float_stream_reference_uses_the_rounded_values(box):
    o, x, aux = box
    o32 = o.with_float_F()
    y = R.product64(o32, "F_INNER", x, None, "lanes16")
    assert not R.compare(R.reference(o32, "F_INNER", x), y)[0]
    assert R.compare(R.reference(o, "F_INNER", x), y)[0]            # ... and the double reference tells the two streams apart


def test_zero_input_gives_exact_zero_or_aux(box):
    o, x, aux = box
    z = np.zeros_like(x)
    for op in NO_S:
        ref = R.reference(o, op, z, aux)
        want = np.zeros_like(x)
        if op in R.NEEDS_AUX:
            sl = slice(0, o.n_u) if op in R.U_OPS else slice(o.n_u, None)
            want[sl] = -aux[sl] if op == "B_MINUS_R" else aux[sl]
        assert np.array_equal(ref.y.astype(np.float64), want)
        assert not R.compare(ref, want)[0]


def test_unit_vectors_give_the_columns(box):
    o, x, aux = box
    for op in ("F", "MASS", "B", "G", "SADDLE"):
        for j in (0, o.n_u - 1, o.n_u, o.n_u + o.n_p - 1):
            e = np.zeros_like(x)
            e[j] = 1.0
            assert np.array_equal(R.product64(o, op, e), R.column(o, op, j)), (op, j)


def _mutated(o, **kw):
    m = R.Operators.__new__(R.Operators)
    m.__dict__.update(o.__dict__)
    m.__dict__.update(kw)
    return m


def test_wrong_products_leave_the_bound(box):
    """one dropped last entry of one row, a column index shifted by one, the wrong sign of the fused subtraction, aux taken from the
    neighbouring row: each fails, and fails only where it is wrong"""
    o, x, aux = box
    row = int(np.argmax(np.diff(o.rp)))              # the longest row: more than 64 entries, the tail loop's business on the device
    # 1. the last entry of one row of F is dropped (as a tail loop that ends one trip early would)
    F = o.F.copy()
    assert F[o.rp[row + 1] - 1] != 0
    F[o.rp[row + 1] - 1] = 0.0
    for op in ("F", "F_RESID", "SADDLE"):
        msgs, _ = R.compare(R.reference(o, op, x, aux), R.product64(_mutated(o, F=F), op, x, aux, "lanes16"))
        assert 1 <= len(msgs) <= o.dim, (op, msgs)
    # ... and of one row of B and of G
    for name, op in (("B", "R_MINUS_B"), ("G", "G_ACC")):
        rp, ci, v = getattr(o, name)
        v = v.copy()
        r = int(np.argmax(np.add.reduceat(np.abs(v), rp[:-1])))         # (rows of constrained dofs are all zero)
        k = rp[r] + int(np.nonzero(v[rp[r]:rp[r + 1]])[0][-1])           # the last entry of the row that is not a stored zero
        v[k] = 0.0
        msgs, _ = R.compare(R.reference(o, op, x, aux), R.product64(_mutated(o, **{name: (rp, ci, v)}), op, x, aux))
        assert len(msgs) == 1, (op, msgs)
    # 2. one column index shifted by one (a wrong lidx / ucols entry)
    ci = o.ci.copy()
    k = o.rp[row] + 1
    ci[k] += 1 if ci[k] + 1 < o.n2 else -1
    msgs, _ = R.compare(R.reference(o, "F", x), R.product64(_mutated(o, ci=ci), "F", x, None, "reversed"))
    assert 1 <= len(msgs) <= o.dim, msgs
    # 3. the wrong sign of the fused subtraction
    for op, other in (("B_MINUS_R", "R_MINUS_B"), ("R_MINUS_B", "B_MINUS_R")):
        msgs, _ = R.compare(R.reference(o, op, x, aux), R.product64(o, other, x, aux))
        assert msgs
    msgs, _ = R.compare(R.reference(o, "F_RESID", x, aux), -R.product64(o, "F_RESID", x, aux))
    assert msgs
    # 4. aux taken from the neighbouring row
    for op in ("F_RESID", "B_MINUS_R", "R_MINUS_B", "G_ACC"):
        msgs, _ = R.compare(R.reference(o, op, x, aux), R.product64(o, op, x, np.roll(aux, 1)))
        assert msgs, op
    # a relative perturbation of one part in 2^40 of a single entry is seen as well; one ulp of the result is not
    y = R.product64(o, "F", x)
    ref = R.reference(o, "F", x)
    i = int(np.argmax(np.abs(y)))
    assert not R.compare(ref, np.where(np.arange(len(y)) == i, np.nextafter(y, np.inf), y))[0]
    assert R.compare(ref, np.where(np.arange(len(y)) == i, y * (1 + 2.0 ** -40), y))[0]


def test_chunk_table_restatement_on_the_crafted_rank_tables():
    """spmv_chunks restated: the tables of the GPU cases give chunks of exactly 1, 15, 16, 17, 31, 32, 33, 447 and 448 rows, a 449-row rank
    cut into 224 + 225, an empty rank that leaves no trace, and the documented fall-backs"""
    for n, need in ((4806, {1, 15, 16, 17, 31, 32, 33, 447, 448, 224, 225}), (1364, {1, 17, 33, 448})):
        ptr = R.crafted_ranks(n, **R.CRAFTED[n])
        assert ptr[0] == 0 and ptr[-1] == n and np.all(np.diff(ptr) >= 0) and np.any(np.diff(ptr) == 0)
        sizes = list(np.diff(R.spmv_chunks(n, ptr, 448)))
        assert sizes == R.CRAFTED_SIZES[n] and need <= set(sizes) and max(sizes) == 448 and sum(sizes) == n
        # ranks of 16 rows at NSX_SPMV_R = 16: a chunk per rank
        b16 = R.spmv_chunks(n, R.block_ptr(n, 16), 16)
        assert len(b16) - 1 == -(-n // 16) and set(np.diff(b16)) == {16, n % 16}
        # no rank table: 128 rows; the default target with ~85-row ranks: one rank per chunk (two would pass 130 rows)
        assert set(np.diff(R.spmv_chunks(n, None))) == {128, n % 128}
        d85 = np.diff(R.spmv_chunks(n, R.block_ptr(n, 85)))
        assert set(d85[:-1]) == {85} and d85[-1] in (n % 85, 85 + n % 85)      # (a short last rank joins its neighbour)
    # ranks of 300 rows at the default target are cut into three parts of 100; a 900-row rank alone (average above 4 x 130) falls back to 128
    assert list(np.diff(R.spmv_chunks(600, [0, 300, 600]))) == [100] * 6
    assert list(np.diff(R.spmv_chunks(1800, [0, 900, 1800]))) == [128] * 14 + [8]
    # NSX_SPMV_R is clamped to 16 .. 448
    assert np.array_equal(R.spmv_chunks(4806, R.block_ptr(4806, 16), 1), R.spmv_chunks(4806, R.block_ptr(4806, 16), 16))
    assert max(np.diff(R.spmv_chunks(4806, R.block_ptr(4806, 600), 10000))) <= 448


def test_chunk_stats_on_a_small_graph():
    rp, ci = np.array([0, 2, 3, 3, 6]), np.array([0, 3, 1, 0, 2, 3])
    n, rows, cols, lists = R.chunk_stats(rp, ci, np.array([0, 2, 4]))
    assert (n, rows, cols) == (2, 2, 3) and [list(c) for c in lists] == [[0, 1, 3], [0, 2, 3]]
