"""GPU suite: every kernel of the Krylov drivers' BLAS-1 layer (csrc/nsx_blas.hip, k_reciprocal of csrc/nsx_solve.hip) DIRECTLY against an
extended-precision restatement of the same operation (tests/blas_reference.py, bounds derived there), through the test hook
nsx_blas1_run -- short programs of the very host functions the solvers call, because what is under test is a reduction followed by a
consumer that sums its partial sums, with or without a finalisation in between.

Kernels and the tests that run them (profile scope in brackets; RAN collects them, the closing test asserts the list)
  k_reduce<OP_DOT>           [dot]           test_every_op_on_every_span, test_fixed_grid_of_a_communicator, test_dot_probes_and_cancellation
  k_reduce<OP_ADD_AND_DOT>   [add_and_dot]   test_every_op_on_every_span, test_chains (w == d and w != d, coefficient from a slot)
  k_axpby                    [axpby]         test_every_op_on_every_span (add, add_dev, sadd, scale, scale_dev_inv), test_chains (cg_direction)
  k_scale_vec                [scale_vec]     test_every_op_on_every_span (plain program)
  k_reciprocal               (no scope)      test_every_op_on_every_span (plain program): its result is compared
  k_axpy_multi               [axpy_multi]    test_multi_axpy (k = 33, 40: two launches)
  k_axpy_multi_from          [axpy_multi]    test_multi_axpy
  k_axpy_multi_zero          [axpy_multi]    test_multi_axpy (with and without y, y aliasing x)
  k_cg_update                [cg_update]     test_every_op_on_every_span (plain program), test_chains
  k_finalize                 (no scope)      test_chains ("final", "mixed"), test_stale_state: bitwise the values k_publish gives
  k_publish                  (no scope)      every read; test_read_range: 64 slots, twice back to back

Lengths, one GPU (blas_reference.SIZES): 1, 63, 64, 255, 256, 257, 1023; 1024 (one workgroup: the value goes straight to the slot); 1025
(two partial sums); 64 * 1024 + 1 (65: the second load of slot_value); 511 * 1024 + 1, 512 * 1024; 512 * 1024 + 257 (the tail loop of k_reduce
and k_cg_update behind the 4-fold prologue).  With a 1-rank communicator (256 partial sums whatever the length): 1, 257, 256 * 256 + 1,
256 * 1024 + 1 (the tail loop).  Spans (split, gap): (n, 0), (0, 7), (1, 7), (256, 512), (300, 7), (1024, 1), (n - 1, 7) where they exist;
the three longest lengths leave out (0, 7) and (1, 7).  The gap holds a NaN with a recognisable payload: after every program it is
bitwise untouched and every sum is finite.

Largest measured error / derived bound per kernel on the MI355X, over every case of this file (recorded as "blas1_unit"):
  k_reduce<OP_DOT> 0.044 (n = 255)          k_reduce<OP_ADD_AND_DOT> 0.250     k_cg_update 0.250       k_axpby 0.495
  k_scale_vec 0.250     k_reciprocal 0.250  k_axpy_multi 0.321 (n = 524 545)   k_axpy_multi_from 0.250 k_axpy_multi_zero 0.250
0.25 is half an ulp of one correctly rounded operation under 2 eps; 0.495 a product and a sum.  No kernel bug was found.  59 tests."""
import numpy as np
import pytest

import blas_reference as R
from conftest import Problem, record

pytestmark = pytest.mark.gpu

RAN = set()
WORST = {}
SCOPES = ("dot", "add_and_dot", "axpby", "scale_vec", "axpy_multi", "cg_update")


@pytest.fixture(scope="module")
def prob():
    return Problem("cylinder", 2, 1)   # the smallest cylinder mesh: the handle only lends its stream and scalar slots


@pytest.fixture(scope="module")
def dev(prob):
    d = prob.device()
    d.profile(True)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev_comm(prob):
    d = prob.device()
    d.comm_init_single()
    d.profile(True)
    yield d
    d.close()


def launches(dev):
    t = dev.profile_table()
    return {k: t.get(k, {}).get("launches", 0) for k in SCOPES}


def expected_launches(ops):
    want = dict.fromkeys(SCOPES, 0)
    for op in ops:
        k = op["kind"]
        if k in ("dot", "add_and_dot", "scale_vec", "cg_update"):
            want[k] += 1
        elif k in ("add", "add_dev", "sadd", "scale", "scale_dev_inv", "cg_direction"):
            want["axpby"] += 1
        elif k == "axpy_multi":
            want["axpy_multi"] += R.cdiv(len(op["vs"]), R.MULTI_MAX)
        elif k == "axpy_multi_into":
            want["axpy_multi"] += 1
    return want


def run(dev, ops, W0, split, gap):
    """the program on the device, with the scopes it must have opened asserted: (vectors, out, scalars)"""
    dev.profile_reset()
    Wd, out, sc = dev.blas1_run(W0, ops, split=split, gap=gap)
    got, want = launches(dev), expected_launches(ops)
    assert got == want, (got, want)
    state = dev.persistent_state()
    assert state["fallbacks"] == 0 and state["dirty_mailbox_words"] == 0, state
    return Wd, out, sc


def check(dev, ops, W0, split, gap, comm, tag, slot_values=None):
    Wd, out, sc = run(dev, ops, W0, split, gap)
    fails, ratios = R.compare(ops, W0, Wd, out, sc, split, gap, comm, slot_values)
    print("blas1_unit", tag, {k: "%.3f" % v for k, v in ratios.items()}, fails)
    for k, v in ratios.items():
        if v > WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, tag)
    assert not fails, "%s: %s" % (tag, fails)
    return Wd, out, sc


def with_published_values(dev, ops, W0, split, gap, comm, tag):
    """the program that publishes every reduction at once, then the program as it is, compared with the slot values the first one
    published (each of them against its extended-precision sum): bitwise the same vectors -- a consumer that sums the partial sums
    sees what the publication saw"""
    twin = R.published_twin(ops)
    Wt, tout, _ = run(dev, twin, W0, split, gap)
    Wd, out, sc = check(dev, ops, W0, split, gap, comm, tag, R.slot_values_from(twin, tout))
    assert R.same_bits(Wd, Wt), tag
    return Wd, out, sc


def spans_for(n):
    sp = R.spans(n)
    return sp if n <= 64 * 1024 + 1 else [s for s in sp if s in ((n, 0), (256, 512), (300, 7), (1024, 1), (n - 1, 7))]


def span_and_plain_programs(dev, n, comm):
    for split, gap in spans_for(n):
        ops, m = R.span_program()
        W0 = R.to_layout(R.gauss(m, n), split, gap)
        with_published_values(dev, ops, W0, split, gap, comm, "n=%d span=(%d,%d) comm=%d" % (n, split, gap, comm))
    RAN.update({"k_reduce<OP_DOT>", "k_reduce<OP_ADD_AND_DOT>", "k_axpby", "k_publish"})
    if n >= 2:
        ops, m = R.plain_program()
        with_published_values(dev, ops, R.to_layout(R.gauss(m, n), n, 0), n, 0, comm, "n=%d plain comm=%d" % (n, comm))
        RAN.update({"k_scale_vec", "k_reciprocal", "k_cg_update"})


@pytest.mark.parametrize("n", R.SIZES)
def test_every_op_on_every_span(dev, n):
    span_and_plain_programs(dev, n, False)


@pytest.mark.parametrize("n", R.SIZES_COMM)
def test_fixed_grid_of_a_communicator(dev_comm, n):
    """256 partial sums per reduction whatever the length, all-reduced over RCCL, consumed as on one GPU"""
    span_and_plain_programs(dev_comm, n, True)


@pytest.mark.parametrize("n", [n for n in R.SIZES if n >= 2])
def test_dot_probes_and_cancellation(dev, n):
    """a = e_i: the dot returns b_i bit for bit, for i at the edges of a workgroup, of the span's split and of the vector; and a dot
    product that cancels to 1e-12 of sum |a_i b_i| stays within the bound relative to that sum"""
    for split, gap in spans_for(n):
        probes = sorted({i for i in (0, 255, 256, split - 1, split, n - 1) if 0 <= i < n})
        V = np.zeros((1 + len(probes), n))
        V[0] = R.gauss(1, n)[0]
        for j, i in enumerate(probes):
            V[1 + j, i] = 1.0
        ops = [dict(kind="dot", d=1 + j, w=0, slot=R.READ_SLOT0 + j, read=1) for j in range(len(probes))]
        ops += [dict(kind="dot", d=0, w=1 + j, slot=R.READ_SLOT0 + j) for j in range(len(probes))]       # the other way round, left in partial sums
        ops += [dict(kind="read", slot=R.READ_SLOT0, count=len(probes))]
        Wd, out, sc = check(dev, ops, R.to_layout(V, split, gap), split, gap, False, "probes n=%d span=(%d,%d)" % (n, split, gap))
        for j, i in enumerate(probes):
            assert R.same_bits(out[j], V[0, i]) and R.same_bits(sc[j], V[0, i]), (n, split, gap, i, out[j], sc[j], V[0, i])
        a, b = R.cancelling(n)
        al, bl = a.astype(R.LD), b.astype(R.LD)
        assert abs(np.sum(al * bl)) < 1e-11 * np.sum(np.abs(al * bl))
        check(dev, [dict(kind="dot", d=0, w=1, slot=R.A, read=1)], R.to_layout(np.stack([a, b]), split, gap), split, gap, False,
              "cancelling n=%d span=(%d,%d)" % (n, split, gap))
    RAN.add("k_reduce<OP_DOT>")


def chains(dev, n, spanned, comm):
    split, gap = (300, 7) if spanned else (n, 0)
    progs, m = R.chain_programs(spanned)
    W0 = R.to_layout(R.gauss(m, n), split, gap)
    tag = "chain n=%d spanned=%d comm=%d " % (n, spanned, comm)
    Wp, pout, psc = check(dev, progs["published"], W0, split, gap, comm, tag + "published")
    values = R.slot_values_from(progs["published"], pout)
    for name in ("partials", "final", "mixed"):
        Wd, out, sc = check(dev, progs[name], W0, split, gap, comm, tag + name, values)
        assert R.same_bits(Wd, Wp) and R.same_bits(sc, psc), tag + name
    RAN.update({"k_finalize", "k_publish", "k_reduce<OP_ADD_AND_DOT>" if spanned else "k_cg_update"})


@pytest.mark.parametrize("spanned", [True, False])
@pytest.mark.parametrize("n", (1025, 64 * 1024 + 1, 512 * 1024 + 257))
def test_chains(dev, n, spanned):
    """dot into A, dot into B, consumers of c * A / B: both slots still in partial sums, both final, one of each, published one by one --
    bitwise the same vectors and values, within the bounds"""
    chains(dev, n, spanned, False)


@pytest.mark.parametrize("spanned", [True, False])
def test_chains_with_a_communicator(dev_comm, spanned):
    chains(dev_comm, 256 * 256 + 1, spanned, True)


@pytest.mark.parametrize("n", (1025, 64 * 1024 + 1, 512 * 1024 + 257))
def test_stale_state(dev, n):
    """the partial sums a long dot left in a slot must be forgotten when a one-workgroup dot or write_scalar rewrites the slot"""
    split, gap = 300, 7
    progs, m = R.stale_programs(min(1000, split))
    W0 = R.to_layout(R.gauss(m, n), split, gap)
    for name, ops in progs.items():
        with_published_values(dev, ops, W0, split, gap, False, "stale %s n=%d" % (name, n))


def test_stale_state_with_a_communicator(dev_comm):
    split, gap, n = 300, 7, 256 * 256 + 1
    progs, m = R.stale_programs(min(1000, split))
    W0 = R.to_layout(R.gauss(m, n), split, gap)
    for name, ops in progs.items():
        with_published_values(dev_comm, ops, W0, split, gap, True, "stale %s comm" % name)


@pytest.mark.parametrize("comm", [False, True])
def test_read_range(dev, dev_comm, comm):
    """read_scalars over 64 slots, final and partial ones mixed, twice back to back: the same 64 values bit for bit"""
    d = dev_comm if comm else dev
    n, split, gap = 64 * 1024 + 1, 1024, 1
    ops, m = R.read_range_program(1000)
    Wd, out, sc = check(d, ops, R.to_layout(R.gauss(m, n), split, gap), split, gap, comm, "read range comm=%d" % comm)
    assert len(sc) == 2 * R.READ_COUNT and R.same_bits(sc[:R.READ_COUNT], sc[R.READ_COUNT:])
    assert np.all(np.isfinite(sc))
    RAN.add("k_publish")


def test_argument_errors_are_the_library_s_own(dev):
    from navierstokes_project_nm4pde_amd.nsx import NsxError
    n = 257
    W0 = R.to_layout(R.gauss(40, n), n, 0)
    vs33, c33 = list(range(2, 35)), [0.5] * 33
    bad = [[dict(kind="axpy_multi_into", d=0, vs=vs33, coef=c33)],
           [dict(kind="axpy_multi_into", d=0, v=1, w=36, vs=[2], coef=[1.0])],
           [dict(kind="read", slot=R.READ_SLOT0, count=65)],
           [dict(kind="finalize", slot=R.READ_SLOT0, count=65)]]
    for ops in bad:
        with pytest.raises(NsxError) as e:
            dev.blas1_run(W0, [dict(kind="dot", d=0, w=1, slot=R.A)] + ops, split=n, gap=0)
        assert e.value.code == -1, ops
        # nothing is left behind: the slot the failed program left in partial sums does not reach the next one
        ops2 = [dict(kind="write_scalar", slot=R.B, a=2.0), dict(kind="scale_dev_inv", d=0, den=R.B)]
        Wd, _, _ = run(dev, ops2, W0, n, 0)
        assert R.same_bits(Wd[0], 0.5 * W0[0])


@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("n", (1025, 64 * 1024 + 1))
def test_multi_axpy(dev, n, k):
    """k = 0, 1, 28, 32 in one launch, 33 and 40 in two; and the documented bitwise identities of the three forms"""
    split, gap = 300, 7
    progs, m = R.multi_programs(k)
    W0 = R.to_layout(R.gauss(m, n), split, gap)
    got = {}
    for name, (ops, row) in progs.items():
        Wd, _, _ = check(dev, ops, W0, split, gap, False, "multi %s k=%d n=%d" % (name, k, n))
        got[name] = Wd[row]
    RAN.add("k_axpy_multi")
    if k <= R.MULTI_MAX:
        assert R.same_bits(got["from"], got["self"])                      # into(x0) == copy, then v_axpy_multi
        Z = W0.copy()
        Z[0][R.index(n, split, gap)] = 0.0
        Wz, _, _ = run(dev, progs["self"][0], Z, split, gap)
        assert R.same_bits(Wz[0], got["zero"])                            # into(zero) == v_axpy_multi on a zeroed x
        assert R.same_bits(got["zero_y"], got["zero_then_sadd"])          # into(zero, y) == into(zero), then y.sadd(-1, 1, x)
        assert R.same_bits(got["zero_y_alias"], got["zero_then_sadd"])    # ... with y aliasing x
        RAN.update({"k_axpy_multi_from", "k_axpy_multi_zero"})


def test_multi_axpy_two_launches_on_a_long_vector(dev):
    n, split, gap = 512 * 1024 + 257, 300, 7
    progs, m = R.multi_programs(33)
    check(dev, progs["self"][0], R.to_layout(R.gauss(m, n), split, gap), split, gap, False, "multi self k=33 n=%d" % n)


def test_every_kernel_has_run():
    want = {"k_reduce<OP_DOT>", "k_reduce<OP_ADD_AND_DOT>", "k_axpby", "k_scale_vec", "k_reciprocal", "k_axpy_multi", "k_axpy_multi_from",
            "k_axpy_multi_zero", "k_cg_update", "k_finalize", "k_publish"}
    for line in __doc__.splitlines():
        if line.startswith("  k_"):
            assert line.split()[0] in want, line
    record("blas1_unit", **{"max_" + k: v for k, (v, _) in WORST.items()}, **{"at_" + k: t for k, (_, t) in WORST.items()})
    missing = sorted(want - RAN)
    assert not missing, missing
    assert set(WORST) >= want - {"k_finalize", "k_publish"}, sorted(WORST)
    assert all(v <= 1.0 for v, _ in WORST.values()), WORST
