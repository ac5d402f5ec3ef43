"""CPU suite: the extended-precision reference of the Gram-Schmidt sweep tests (tests/mgs_reference.py) is right, and its comparison
bites: deliberately broken restatements of a sweep -- the ways a kernel of csrc/nsx_mgs.hip can be subtly wrong -- FAIL it at every
vector length the GPU module (tests/test_gpu_mgs_sweep.py) uses, with the margin K that module asserts with."""
import numpy as np
import pytest

import mgs_reference as R

# lengths with at least three vectors in the cycle: below (n = 1, 2: ONE vector, no sweep at all) most of the operations broken
# here do not exist, and the GPU module's cases there check the norm and the scaling of vector 0 only
MUTATION_SIZES = [n for n in R.ALL_SIZES if R.basis_length(n) >= 3]
SENTINEL = -7.0e300


def _ref(n, kind="gauss"):
    return R.reference(n, R.basis_length(n), R.SEED, kind)


def _span(n):
    return n // 3, 37


def _cycle64(ref, **wrong):
    with np.errstate(invalid="ignore", divide="ignore"):   # a broken sweep may well produce a negative |w'|^2
        return R.chain(ref.V, np.float64, **wrong)


def _check(ref, Q, H, after, before, split, gap, normalized=None, **kw):
    W = R.to_layout(np.asarray(Q, dtype=np.float64), split, gap, SENTINEL)
    normalized = np.ones(ref.m, dtype=np.int32) if normalized is None else normalized
    return R.compare(ref, W, np.asarray(H, dtype=np.float64), np.asarray(after, dtype=np.float64), np.asarray(before, dtype=np.float64),
                     normalized, split=split, gap=gap, sentinel=SENTINEL, consider=True, formula=True,
                     expect_normalized=np.ones(ref.m, dtype=np.int32), **kw)


# ---- the reference itself
@pytest.mark.parametrize("n", [64, 257, 5000, 100001])
def test_reference_against_a_qr_factorisation(n):
    """Gram-Schmidt IS a QR factorisation V^T = Q^T-columns times R with a positive diagonal: Q, the coefficients and the norms of
    the extended-precision chain against Householder QR (float64, backward stable: errors of cond * eps, cond <= 10)."""
    ref = _ref(n)
    assert R.condition_number(ref.V) <= 10
    q, r = np.linalg.qr(ref.V.T)
    sign = np.sign(np.diag(r))
    q, r = q * sign, (r.T * sign).T
    tol = 200 * R.EPS * 10
    assert np.abs(np.asarray(ref.Q, dtype=np.float64) - q.T).max() <= tol * np.abs(q).max()
    for k in range(ref.m):
        assert abs(float(np.sqrt(ref.after[k])) - r[k, k]) <= tol * r[k, k]
        assert abs(float(ref.before[k]) - ref.V[k] @ ref.V[k]) <= tol * float(ref.before[k])
        if k:
            assert np.abs(np.asarray(ref.H[k, :k], dtype=np.float64) - r[:k, k]).max() <= tol * np.sqrt(float(ref.before[k]))


@pytest.mark.parametrize("n", R.ALL_SIZES)
def test_inputs_are_well_conditioned(n):
    m = R.basis_length(n)
    assert R.condition_number(R.make_vectors(n, m, R.SEED)) <= 10
    if m >= 3:
        assert R.condition_number(R.make_vectors(n, m, R.SEED, "dependent")[:m - 1]) <= 10


def test_reference_is_extended_precision_and_orthonormal_beyond_float64():
    ref = _ref(5000)
    assert ref.Q.dtype == np.longdouble and np.finfo(ref.Q.dtype).eps < 1e-18
    G = ref.Q @ ref.Q.T
    assert float(np.max(np.abs(G - np.eye(ref.m)))) < 1e-17   # cond * eps_longdouble; a float64 chain reaches 1e-15


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [63, 1025, 3073, 100001])
def test_float64_chain_passes_the_comparison(n, kind):
    """a correct float64 implementation passes with K = 2 already (its ratios are <= 1 by construction): nothing right is refused"""
    ref = _ref(n, kind)
    for split, gap in [(n, 0), _span(n), (0, 5), (n - 1, 1)]:
        failures, ratios = _check(ref, *_cycle64(ref), split, gap, k_margin=2.0)
        assert not failures, failures
        assert max(ratios.values()) <= 1.0


def test_dependent_vector_is_what_it_claims():
    ref = _ref(5000, "dependent")
    k = ref.m - 1
    left = float(np.sqrt(ref.after[k] / ref.before[k]))
    assert 0.3e-9 < left < 3e-9                      # far below SolverGMRES' threshold 10 sqrt(eps) = 1.5e-7 ...
    assert R.condition_number(ref.V[:k]) <= 10       # ... on a well-conditioned basis
    assert all(float(np.sqrt(ref.after[j] / ref.before[j])) > 0.1 for j in range(1, k))


def test_yardstick_is_of_rounding_size():
    """err64 per quantity is a few eps (a yardstick of 1e-12 would let a wrong kernel through)"""
    for n in (65, 2561, 100001):
        e = _ref(n).err64
        assert e["q"] < 1e-14 and e["h"] < 2e-15 and e["after"] < 2e-15 and e["before"] < 2e-15 and e["orth"] < 1e-14, e
        assert max(R.bounds(_ref(n), True).values()) < R.HARD_LIMIT


# ---- mutations: each must FAIL, at every length, with the final K
def _must_fail(ref, out, split, gap, what, **kw):
    failures, _ = _check(ref, *out, split, gap, **kw)
    assert failures, "%s passed the comparison at n = %d" % (what, ref.n)


@pytest.mark.parametrize("n", MUTATION_SIZES)
def test_broken_sweeps_fail_the_comparison(n):
    ref = _ref(n)
    split, gap = _span(n)
    good = _cycle64(ref)
    assert not _check(ref, *good, split, gap)[0]
    # one entry left out of every dot product: a thread's tail entry, the first entry, the first entry behind the gap
    for entry, what in ((n - 1, "last entry dropped"), (0, "first entry dropped"), (split, "entry at split dropped")):
        _must_fail(ref, _cycle64(ref, drop=entry), split, gap, what)
    # one entry not updated by w -= h v
    _must_fail(ref, _cycle64(ref, stale=n - 1), split, gap, "tail entry not updated")
    _must_fail(ref, _cycle64(ref, stale=split), split, gap, "entry at split not updated")
    # the newest row of the Gram matrix one column short
    _must_fail(ref, _cycle64(ref, gram_short=True), split, gap, "Gram row one column short")
    Q, H, after, before = (x.copy() for x in good)
    # gap entries overwritten (one of them, by one bit pattern that is still a number)
    W = R.to_layout(Q, split, gap, SENTINEL)
    W[ref.m - 1, split + gap - 1] = 0.0
    failures, _ = R.compare(ref, W, H, after, before, np.ones(ref.m, np.int32), split=split, gap=gap, sentinel=SENTINEL, consider=True, formula=True)
    assert failures, "overwritten gap passed at n = %d" % n
    # coefficients of links i and i + 1 swapped (the last sweep's first two)
    Hs = H.copy()
    Hs[ref.m - 1, [0, 1]] = Hs[ref.m - 1, [1, 0]]
    _must_fail(ref, (Q, Hs, after, before), split, gap, "swapped coefficients")
    # |w|^2 before the sweep in the place of |w|^2 after it
    wrong = after.copy()
    wrong[1:] = before[1:]
    _must_fail(ref, (Q, H, wrong, before), split, gap, "norm before in the place of the norm after")
    # the sweep's own decision reported wrongly
    flags = np.ones(ref.m, np.int32)
    flags[ref.m - 1] = 0
    _must_fail(ref, good, split, gap, "wrong normalized flag", normalized=flags)


@pytest.mark.parametrize("n", [1, 2])
def test_broken_norm_of_a_single_vector_fails(n):
    """one vector, no sweep: what can be wrong is the norm of vector 0 and its scaling"""
    ref = _ref(n)
    assert ref.m == 1
    good = _cycle64(ref)
    assert not _check(ref, *good, n, 0)[0]
    _must_fail(ref, _cycle64(ref, drop=n - 1), n, 0, "last entry dropped")
    Q, H, after, before = (x.copy() for x in good)
    _must_fail(ref, (Q * (1 + 1e-9), H, after, before), n, 0, "scaled wrongly")
