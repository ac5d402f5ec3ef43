"""CPU suite: tests/stats_reference.py -- the numpy restatement of the running statistics' contract (include/nsx.h, "running statistics")
that tests/test_gpu_stats.py holds the device against -- pinned by closed forms, by a two-pass mean / covariance, and by the rounding bounds
of its float64 run against its long-double run.

The bounds.  u = 2^-53, n samples, X_i = max_k |x_k,i| per DoF, W = sum w.  Both runs take the same double coefficients r, q, so those
count as exact.  Per sample the device rounds

    d_i  = (x_i - m_i)(1 + e1)
    m_i' = (m_i + (r d_i)(1 + e2))(1 + e3)
    C_ij' = (C_ij + ((q d_i)(1 + e4) d_j)(1 + e5))(1 + e6),        |e| <= u.

Mean: the exact step is m' = (1 - r) m + r x with 0 < r <= 1, a convex combination, so |m| <= X, |d| <= 2 X, and an error E of m is damped
to (1 - r) E.  The three roundings add at most r |d| u + r |d| u + |m'| u <= (4 r + 1) u X <= 5 u X.  After n samples |E| <= 5 n u X.
Co-moment: nothing damps or amplifies an error of C.  Sample k adds (a) the error of d in the product: |delta d_i| <= |E_i| + 2 u X_i <=
(5 (k - 1) + 2) u X_i, so q (|delta d_i| |d_j| + |d_i| |delta d_j|) <= q (20 (k - 1) + 8) u X_i X_j; (b) the two roundings of the product,
2 u q |d_i| |d_j| <= 8 u q X_i X_j; (c) the rounding of the sum, u |C_ij'| <= u W X_i X_j (Cauchy-Schwarz and C_ii <= sum w x_i^2).  With
sum_k q_k <= sum_k w_k = W (q_k = W_{k-1} w_k / W_k <= w_k) the total is (20 (n - 1) + 16 + n) u W X_i X_j = (21 n - 4) u W X_i X_j to first
order in u.  The tests use (24 n + 16) u W X_i X_j, the figure the feature was specified with: it lies above the derived one for every n and
leaves room for the terms of second order and for the long-double run's own rounding (2^-11 u per operation).
The diagonal never decreases in either run: q >= 0 and (q d) d has the sign of d^2 after any monotone rounding."""
import numpy as np
import pytest

import stats_reference as SR


def test_long_double_is_an_extended_format():
    assert SR.LONG_OK and np.finfo(np.longdouble).nmant >= 63              # what makes the long-double run a reference


def series(seed, n_samples, n, nc, offset=0.0, amp=1.0):
    rng = np.random.default_rng(seed)
    return offset + amp * rng.standard_normal((n_samples, n, nc))


def test_plane_order_and_coefficients():
    assert SR.pairs(1) == [(0, 0)]
    assert SR.pairs(2) == [(0, 0), (1, 1), (0, 1)]
    assert SR.pairs(3) == [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    W1, r, q = SR.update_coefficients(0.0, 0.3)
    assert (W1, r, q) == (0.3, 1.0, 0.0)                                  # the first sample: r = 1, q = 0 exactly
    W1, r, q = SR.update_coefficients(0.3, 0.2)
    assert W1 == 0.3 + 0.2 and r == 0.2 / (0.3 + 0.2) and q == 0.3 * (0.2 / (0.3 + 0.2))


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_first_sample_and_constant_series(dtype):
    x = series(1, 1, 37, 3)[0]
    a = SR.Accumulator(37, 3, dtype).add(x, 0.7)
    assert np.array_equal(a.m, x.astype(dtype)) and not a.C.any()          # m = x, C = 0 exactly
    for w in (0.7, 1e-3, 5.0, 0.1):
        a.add(x, w)
    assert np.array_equal(a.m, x.astype(dtype)) and not a.C.any()          # a constant series: d = 0 in every step
    assert a.samples == 5 and a.W == (((0.7 + 0.7) + 1e-3) + 5.0) + 0.1


@pytest.mark.parametrize("nc", [1, 2, 3])
def test_long_double_recurrence_against_two_passes(nc):
    xs, ws = series(2, 9, 50, nc), np.random.default_rng(3).uniform(0.2, 2.0, 9)
    a = SR.run(xs, ws, dtype=np.longdouble)[0]
    mean, C, W = SR.two_pass(xs, ws)
    assert abs(np.longdouble(a.W) - W) <= 16 * SR.U * W
    scale = np.abs(xs).max()
    assert np.abs(a.m - mean).max() <= 1e-15 * scale
    assert np.abs(a.C - C).max() <= 1e-15 * float(W) * scale ** 2
    assert (a.C[:, :nc] >= 0).all()


@pytest.mark.parametrize("nc", [1, 3])
def test_pooled_bins_against_one_bin(nc):
    xs, ws = series(4, 8, 41, nc, offset=0.5), np.random.default_rng(5).uniform(0.5, 1.5, 8)
    bins = [0, 2, 2, 0, 3, 2, 0, 3]                                         # bin 1 stays empty and is skipped
    one = SR.run(xs, ws, dtype=np.longdouble)[0]
    accs = SR.run(xs, ws, bins, 4, dtype=np.longdouble)
    assert [a.samples for a in accs] == [3, 0, 3, 2]
    before = [(a.m.copy(), a.C.copy()) for a in accs]
    p = SR.pooled(accs)
    assert p.samples == 8 and abs(p.W - one.W) <= 8 * SR.U * one.W
    assert np.abs(p.m - one.m).max() <= 1e-15 and np.abs(p.C - one.C).max() <= 1e-14
    for a, (m, C) in zip(accs, before):
        assert np.array_equal(a.m, m) and np.array_equal(a.C, C)            # the fold leaves the bins alone
    assert SR.pooled([SR.Accumulator(3, nc)]) is None
    assert SR.pooled(accs[:2]) is accs[0]                                    # one non-empty bin: the bin itself


def test_rounding_bounds_float64_against_long_double():
    """60 seeded series, zero-mean ones and ones with a large mean and a small fluctuation, equal and unequal weights"""
    worst_m = worst_C = 0.0
    for seed in range(60):
        rng = np.random.default_rng(100 + seed)
        n_samples, nc = int(rng.integers(2, 40)), int(rng.integers(1, 4))
        offset, amp = ((0.0, 1.0), (1e3, 1e-3), (-7.0, 0.5))[seed % 3]
        xs = series(seed, n_samples, 29, nc, offset, amp)
        ws = np.full(n_samples, 0.01) if seed % 2 else rng.uniform(1e-3, 3.0, n_samples)
        f, l = SR.run(xs, ws)[0], SR.run(xs, ws, dtype=np.longdouble)[0]
        bm, bC = SR.bounds(xs, ws)
        rm, rC = SR.ratio(f.m, l.m, bm), SR.ratio(f.C, l.C, bC)
        assert rm <= 1.0 and rC <= 1.0, (seed, rm, rC)
        assert (f.C[:, :nc] >= 0).all() and (l.C[:, :nc] >= 0).all()        # no negative diagonal
        worst_m, worst_C = max(worst_m, rm), max(worst_C, rC)
    print("largest ratios: mean %.3f, co-moment %.4f" % (worst_m, worst_C))
    assert 0 < worst_m and 0 < worst_C                                       # the runs do differ: the bounds measure something


def test_derived_quantities():
    xs, ws = series(7, 6, 23, 3), np.full(6, 0.25)
    a = SR.run(xs, ws)[0]
    d = SR.derive(a.m, a.C, a.W)
    invW = 1.0 / a.W
    assert np.array_equal(d["stress"], a.C * invW)
    assert np.array_equal(d["rms"], np.sqrt(a.C[:, :3] * invW))
    assert np.array_equal(d["tke"][:, 0], 0.5 * ((a.C[:, 0] * invW + a.C[:, 1] * invW) + a.C[:, 2] * invW))
    ref = SR.derive(a.m, a.C, a.W, np.longdouble)
    for k in d:
        assert SR.ratio(d[k], ref[k], 4 * SR.U * np.abs(ref[k])) <= 1.0, k
