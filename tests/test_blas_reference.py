"""CPU suite: the comparison tests/test_gpu_blas1.py runs on the device (tests/blas_reference.py: compare) accepts a float64 restatement
of the BLAS-1 kernels and rejects every subtly wrong one, on the programs, lengths and spans the GPU tests use.

Mutants of the restatement (blas_reference.MUTANTS) and where each one shows:
  last_partial_dropped     the consumer's sum of the partial sums loses its last term: every length with more than one workgroup
  gap_ignored              logical entry i read at storage i: every span with a gap
  gap_entry_summed         the first gap entry added into a reduction: every span with a gap (the gap holds NaN: the sum is not finite)
  stale_slot               a slot rewritten by a one-workgroup dot or by write_scalar still counts as spread over the old partial sums
  denominator_ignored      c * num / den evaluated as c * num
  multi_above_32_dropped   the second launch of v_axpy_multi missing: k = 33, 40
  y_not_negated            x = y + s instead of -y + s"""
import numpy as np
import pytest

import blas_reference as R

SMALL = tuple(n for n in R.SIZES if n <= 64 * 1024 + 1)
LARGE = tuple(n for n in R.SIZES if n > 64 * 1024 + 1)


def run(ops, W0, split, gap, comm=False, mutant=None, values_from=None):
    """model the program (and its publishing twin for the slot values, unmutated inputs alike), then compare"""
    Wd, out, sc = R.model(ops, W0, split, gap, comm, mutant)
    slot_values = None
    if values_from is not None:
        _, tout, _ = R.model(values_from, W0, split, gap, comm, mutant)
        slot_values = R.slot_values_from(values_from, tout)
    return R.compare(ops, W0, Wd, out, sc, split, gap, comm, slot_values), Wd


def vectors(m, n, split, gap):
    return R.to_layout(R.gauss(m, n), split, gap)


def span_case(n, split, gap, comm=False, mutant=None):
    ops, m = R.span_program()
    (fails, ratios), _ = run(ops, vectors(m, n, split, gap), split, gap, comm, mutant, values_from=R.published_twin(ops))
    return fails, ratios


@pytest.mark.parametrize("n", SMALL)
def test_restatement_passes_on_every_span(n):
    for split, gap in R.spans(n):
        fails, ratios = span_case(n, split, gap)
        assert not fails, (n, split, gap, fails)
        assert all(0 <= r <= 1 for r in ratios.values())
    if n >= 2:
        ops, m = R.plain_program()
        (fails, _), _ = run(ops, vectors(m, n, n, 0), n, 0, values_from=R.published_twin(ops))
        assert not fails, fails


@pytest.mark.parametrize("n", LARGE)
def test_restatement_passes_on_the_long_vectors(n):
    fails, _ = span_case(n, 300, 7)
    assert not fails, fails


@pytest.mark.parametrize("n", R.SIZES_COMM)
def test_restatement_passes_with_the_fixed_grid(n):
    for split, gap in R.spans(n)[:3]:
        fails, _ = span_case(n, split, gap, comm=True)
        assert not fails, (n, split, gap, fails)


def test_the_bound_is_not_idle():
    """the restatement uses a good share of the derived bounds: they are not orders of magnitude too wide"""
    _, ratios = span_case(64 * 1024 + 1, 300, 7)
    assert ratios["k_axpby"] > 0.2 and ratios["k_axpy_multi"] > 0.05 and ratios["k_reduce<OP_DOT>"] > 1e-3, ratios


def test_cancelling_dot_is_measured_against_the_sum_of_magnitudes():
    n = 64 * 1024 + 1
    a, b = R.cancelling(n)
    al, bl = a.astype(R.LD), b.astype(R.LD)
    rel = float(abs(np.sum(al * bl)) / np.sum(np.abs(al * bl)))
    assert 1e-13 < rel < 1e-11, rel
    W0 = R.to_layout(np.stack([a, b]), 300, 7)
    ops = [dict(kind="dot", d=0, w=1, slot=R.A, read=1)]
    (fails, ratios), _ = run(ops, W0, 300, 7)
    assert not fails and ratios["k_reduce<OP_DOT>"] <= 1, (fails, ratios)
    (fails, _), _ = run(ops, W0, 300, 7, mutant="last_partial_dropped")
    assert fails


@pytest.mark.parametrize("n,comm", [(1025, False), (64 * 1024 + 1, False), (512 * 1024 + 257, False), (256 * 256 + 1, True), (256 * 1024 + 1, True)])
def test_last_partial_dropped(n, comm):
    fails, _ = span_case(n, 300, 7, comm=comm, mutant="last_partial_dropped")
    # consumer and publication run the same slot_value: the value is what gives the mutant away, against the extended-precision sum
    # (a consumer that ALONE went wrong would differ bitwise from the run that publishes first: the chains of test_gpu_blas1)
    assert any("(value)" in f for f in fails), fails


@pytest.mark.parametrize("mutant", ["gap_ignored", "gap_entry_summed"])
@pytest.mark.parametrize("n", (257, 1025, 64 * 1024 + 1))
def test_gap_mutants(n, mutant):
    for split, gap in R.spans(n):
        if gap == 0:
            continue
        fails, _ = span_case(n, split, gap, mutant=mutant)
        assert fails, (n, split, gap)
    for split, gap in R.spans(257)[1:3]:
        fails, _ = span_case(257, split, gap, comm=True, mutant=mutant)
        assert fails, (split, gap)


@pytest.mark.parametrize("n", (1025, 64 * 1024 + 1, 512 * 1024 + 257))
def test_stale_slot(n):
    split, gap = 300, 7
    progs, m = R.stale_programs(min(1000, split))
    W0 = vectors(m, n, split, gap)
    for name, ops in progs.items():
        twin = R.published_twin(ops)
        (fails, _), good = run(ops, W0, split, gap, values_from=twin)
        assert not fails, (name, fails)
        (_, _), good_twin = run(twin, W0, split, gap)
        assert R.same_bits(good, good_twin)
        Wd, out, sc = R.model(ops, W0, split, gap, mutant="stale_slot")
        _, tout, _ = R.model(twin, W0, split, gap)          # the values an unmutated publication gives
        fails, _ = R.compare(ops, W0, Wd, out, sc, split, gap, slot_values=R.slot_values_from(twin, tout))
        assert fails, name
        assert not R.same_bits(Wd, good), name


@pytest.mark.parametrize("spanned", [True, False])
def test_chains_and_the_ignored_denominator(spanned):
    n = 64 * 1024 + 1
    split, gap = (300, 7) if spanned else (n, 0)
    progs, m = R.chain_programs(spanned)
    W0 = vectors(m, n, split, gap)
    results = {}
    for name, ops in progs.items():
        (fails, _), results[name] = run(ops, W0, split, gap, values_from=progs["published"])
        assert not fails, (name, fails)
    for name in progs:
        assert R.same_bits(results[name], results["partials"]), name
    for name, ops in progs.items():
        (fails, _), _ = run(ops, W0, split, gap, mutant="denominator_ignored", values_from=progs["published"])
        assert fails, name


def test_read_range_mixing_final_and_partial_slots():
    n, split, gap = 64 * 1024 + 1, 1024, 1
    ops, m = R.read_range_program(1000)
    W0 = vectors(m, n, split, gap)
    (fails, ratios), _ = run(ops, W0, split, gap)
    assert not fails, fails
    (fails, _), _ = run(ops, W0, split, gap, mutant="last_partial_dropped")
    assert fails
    Wd, out, sc = R.model(ops, W0, split, gap)
    sc = sc.copy()
    sc[R.READ_COUNT + 5] = np.nextafter(sc[R.READ_COUNT + 5], np.inf)     # the second publication differs from the first in one bit
    fails, _ = R.compare(ops, W0, Wd, out, sc, split, gap)
    assert fails


@pytest.mark.parametrize("k", R.KS)
def test_multi_axpy_and_its_mutants(k):
    n, split, gap = 1025, 300, 7
    progs, m = R.multi_programs(k)
    W0 = vectors(m, n, split, gap)
    got = {}
    for name, (ops, row) in progs.items():
        (fails, _), Wd = run(ops, W0, split, gap)
        assert not fails, (k, name, fails)
        got[name] = Wd[row]
    if k <= R.MULTI_MAX:
        assert R.same_bits(got["zero_y_alias"], got["zero_then_sadd"]) and R.same_bits(got["zero_y"], got["zero_then_sadd"])
        assert R.same_bits(got["from"], got["self"])
        Z = W0.copy()
        Z[0][R.index(n, split, gap)] = 0.0
        (_, _), Wz = run(progs["self"][0], Z, split, gap)
        assert R.same_bits(Wz[0], got["zero"])
        for name in ("zero_y", "zero_y_alias"):
            (fails, _), _ = run(progs[name][0], W0, split, gap, mutant="y_not_negated")
            assert fails, name
    else:
        (fails, _), _ = run(progs["self"][0], W0, split, gap, mutant="multi_above_32_dropped")
        assert fails


def test_depth_is_the_code_s():
    assert R.red_blocks(1024, False) == 1 and R.red_blocks(1025, False) == 2 and R.red_blocks(64 * 1024 + 1, False) == 65
    assert R.red_blocks(512 * 1024 + 257, False) == 512 and R.red_blocks(1, True) == 256
    assert R.depth(1024, 1) == 4 + 10 and R.depth(512 * 1024 + 257, 512) == 5 + 10 + 9   # the fifth term: the tail loop behind the 4-fold prologue
    assert R.depth(256 * 1024 + 1, 256) == 5 + 19
    assert R.ew_blocks(257) == 1 and R.ew_blocks(512 * 1024 + 257) == 1025    # a workgroup per 512 entries: a second grid-stride trip from n = 257 on
