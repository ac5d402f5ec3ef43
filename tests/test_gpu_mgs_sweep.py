"""GPU suite: every variant of the Gram-Schmidt sweep (csrc/nsx_mgs.hip) DIRECTLY against an extended-precision reference of
SolverGMRES' modified Gram-Schmidt chain (tests/mgs_reference.py), through the test hook nsx_gram_schmidt_sweeps -- the vectors that
come back entry by entry, the coefficients, |w'|^2, |w|^2 before the sweep, the sweep's own decision whether it may normalise, and the
gap entries of a block vector's layout bit for bit -- at the edges of every instantiation:

  variants        NSX_MGS=0 (launch-per-link chain on k_reduce), the default one-exchange sweep (k_mgs_one), the two-pass
                  sweep (k_ls_*: a vector too long for the capped grid), and on a 1-rank RCCL communicator the collective inside the
                  grid (k_mgs_one<.., true>), NSX_MGS_DIST=0 (two passes) and NSX_MGS_DIST=0 NSX_MGS_LOWSYNC=0 (chain)
  instantiations  NSX_MGS_MAXWG=1 / 3 force the 8 / 10 / 12 entries-per-thread kernels and the two-pass sweep on short vectors, at
                  n = the last length that fits, and one more; the real grid from one entry to more than 256 workgroups
  basis           30 vectors where the length allows: one cycle passes every dim 1..29, i.e. DMAX and DMAX + 1 of each instantiation
  spans           contiguous, and (split, gap) = (n // 3, 37), (0, 5), (n - 1, 1) with a sentinel in the gap
  flags           consider (far from the threshold, and with a vector the sweep all but annihilates), normalize = false, both
  norm guard      0 / default / 1e300 for the one-exchange sweep (with and without the collective inside) and the two-pass sweep (Gram
                  formula always / guarded / never; never, with the collective inside: every norm through the second collective)

What runs: every handle (variant x grid cap, one per length with a communicator) x its lengths x {4 spans plain; consider,
normalize = false on the (n // 3, 37) span; both on the contiguous one; the annihilated vector with consider where the cycle has >= 3
vectors; and, where |w'|^2 may come from the Gram formula, guards 0 and 1e300 plain and with consider} -- not the full product of
spans x flags x guards.

Every case also checks WHICH kernel ran (profile table, nsx_path_info, nsx_persistent_state).  Tolerances: K x (deviation of a
float64 restatement of the chain from the reference + 4 eps), K measured -- see tests/mgs_reference.py.  Each environment setting
gets a handle of its own (the sweep reads the environment once per handle)."""
import os

import numpy as np
import pytest

import mgs_reference as R
from conftest import Problem, record

pytestmark = pytest.mark.gpu

SENTINEL = -7.0e300
CONSIDER, NO_NORMALIZE = 1, 2
ENV_KEYS = ("NSX_MGS", "NSX_MGS_MAXWG", "NSX_MGS_DIST", "NSX_MGS_LOWSYNC")


@pytest.fixture(scope="module")
def prob():
    return Problem("cylinder", 2, 1)   # the smallest cylinder mesh: the handle only lends its stream, scalar slots and mailboxes


def cdiv(a, b):
    return -(-a // b)


def expected_path(n, env, comm):
    """what v_mgs must run for a vector of n entries: ("chain" | "two_pass" | "sweep", entries per thread or None, workgroups or None) --
    mgs_plan / mgs_pick restated for the grids a test caps (NSX_MGS_MAXWG); the uncapped grid's size is the device's business"""
    if env.get("NSX_MGS") == "0":
        return "chain", None, None
    if comm and env.get("NSX_MGS_DIST") == "0":
        return ("chain" if env.get("NSX_MGS_LOWSYNC") == "0" else "two_pass"), None, None
    es = (8,) if comm else (8, 10, 12)
    cap = int(env["NSX_MGS_MAXWG"]) if "NSX_MGS_MAXWG" in env else None
    if cap is None:
        return "sweep", None, None
    for e in es:
        nwg = max(1, min(cap, cdiv(n, 1024)))
        if cdiv(n, nwg * 256) <= e:
            return "sweep", e, nwg
    return "two_pass", None, None


def cases_for(n, guards):
    """(kind, span, flags, norm_guard) of one vector length"""
    m = R.basis_length(n)
    gapped = (n // 3, 37)
    out = [("gauss", sp, 0, -1.0) for sp in R.spans(n)]
    out += [("gauss", gapped, CONSIDER, -1.0), ("gauss", gapped, NO_NORMALIZE, -1.0), ("gauss", None, CONSIDER | NO_NORMALIZE, -1.0)]
    if m >= 3:
        out.append(("dependent", gapped, CONSIDER, -1.0))
    if guards:
        for g in (0.0, 1e300):
            out += [("gauss", None, 0, g), ("gauss", gapped, CONSIDER, g)]
    return out


def run_handle(prob, env, sizes, comm=False, want_paths=()):
    """all cases of `sizes` on ONE fresh handle created under `env`; returns nothing, asserts at the end with every failure listed"""
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env)
    failures, worst, ran = [], {}, set()
    dev = None
    try:
        dev = prob.device()
        if comm:
            dev.comm_init_single()
        dev.profile(True)
        for n in sizes:
            m = R.basis_length(n)
            path, e_want, nwg_want = expected_path(n, env, comm)
            # the Gram formula for |w'|^2: the one-exchange sweep and the two-pass sweep (unless the guard refuses it always)
            formula_variant = path == "sweep" or path == "two_pass"
            for kind, span, flags, guard in cases_for(n, guards=formula_variant):
                tag = "%s n=%d %s span=%s flags=%d guard=%g" % (env, n, kind, span, flags, guard)
                ref = R.reference(n, m, R.SEED, kind)
                assert ref.cond <= 10, tag
                split, gap = span if span else (n, 0)
                W = R.to_layout(ref.V, split, gap, SENTINEL)
                dev.profile_reset()
                Wd, H, after, before, normalized = dev.gram_schmidt_sweeps(W, split=split, gap=gap, norm_guard=guard, flags=flags)
                table, info, state = dev.profile_table(), dev.path_info(), dev.persistent_state()
                consider, normalize = bool(flags & CONSIDER), not (flags & NO_NORMALIZE)
                # the sweep normalises itself on the persistent path only, and not where SolverGMRES would sweep again (with the
                # collective inside the grid a refused formula leaves the norm to a second collective: not normalised either)
                expect = np.zeros(m, dtype=np.int32)
                if path == "sweep" and normalize:
                    expect[1:] = 1
                    for k in ref.weak:
                        expect[k] = 0
                    if comm and guard > 1e299:   # the formula is always refused: every norm goes through the second collective
                        expect[:] = 0
                fails, ratios = R.compare(ref, Wd, H, after, before, normalized, split=split, gap=gap, sentinel=SENTINEL, consider=consider,
                                          formula=formula_variant and guard < 1e299, expect_normalized=expect)
                print("mgs_sweep_unit", tag, path, info["sweep_entries_per_thread"], info["sweep_grid"], {k: "%.2f" % v for k, v in ratios.items()}, fails)
                failures += ["%s: %s" % (tag, f) for f in fails]
                for q, v in ratios.items():
                    if v > worst.get(q, (-1.0, ""))[0]:
                        worst[q] = (v, tag)
                # ---- the intended kernel really ran
                if m > 1:
                    launches = {k: table.get(k, {}).get("launches", 0) for k in ("mgs_sweep", "mgs_dots", "mgs_update", "add_and_dot")}
                    want = {"sweep": ("mgs_sweep",), "two_pass": ("mgs_dots", "mgs_update"), "chain": ("add_and_dot",)}[path]
                    for name, count in launches.items():
                        if (count > 0) != (name in want):
                            failures.append("%s: %d launches of %s on the %s path" % (tag, count, name, path))
                    if path == "sweep":
                        e, nwg = info["sweep_entries_per_thread"], info["sweep_grid"]
                        ran.add(("sweep", e))
                        if e_want is not None and (e, nwg) != (e_want, nwg_want):
                            failures.append("%s: %d entries per thread on %d workgroups, expected %d on %d" % (tag, e, nwg, e_want, nwg_want))
                        if e_want is None:  # the real grid: the smallest instantiation, a workgroup per 1024 entries up to what is resident
                            if e not in (8, 10, 12) or nwg * 256 * e < n or nwg > 512 or (n <= 100001 and (e, nwg) != (8, cdiv(n, 1024))):
                                failures.append("%s: %d entries per thread on %d workgroups" % (tag, e, nwg))
                            if n >= 300001 and nwg <= 256:
                                failures.append("%s: %d workgroups do not reach the reducers' loop over more than 256 mailboxes" % (tag, nwg))
                        if info["sweep_collective_inside"] != (1 if comm else 0):
                            failures.append("%s: collective inside = %d" % (tag, info["sweep_collective_inside"]))
                        if not state["sweep_persistent"]:
                            failures.append("%s: the handle reports no persistent sweep" % tag)
                    else:
                        ran.add((path, None))
                if state["fallbacks"] != 0 or state["dirty_mailbox_words"] != 0 or info["fallbacks"] != 0:
                    failures.append("%s: fallbacks %d, dirty mailbox words %d" % (tag, state["fallbacks"], state["dirty_mailbox_words"]))
                    break   # a sweep that timed out has switched the handle to another path: nothing more to learn from it
    finally:
        if dev is not None:
            dev.close()
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    record("mgs_sweep_unit", env=str(env), comm=comm, sizes=str(list(sizes)), ran=str(sorted(ran, key=str)),
           **{"max_" + q: v for q, (v, _) in worst.items()}, **{"at_" + q: t for q, (_, t) in worst.items()})
    for p in want_paths if any(R.basis_length(n) > 1 for n in sizes) else ():   # (a single vector is never swept)
        if p not in ran:
            failures.append("%s: %s never ran" % (env, p))
    assert not failures, "\n".join(failures[:40] + (["... %d more" % (len(failures) - 40)] if len(failures) > 40 else []))


def test_chain_of_separate_launches(prob):
    """NSX_MGS=0: v_dot + v_add_and_dot per link (k_reduce), the path every fallback ends on"""
    run_handle(prob, {"NSX_MGS": "0"}, R.SIZES_GRID + (3073,), want_paths=[("chain", None)])


def test_persistent_sweep_on_the_real_grid(prob):
    """k_mgs_one<8,10>: one entry ... more than 256 workgroups in the reducers' mailbox loop"""
    run_handle(prob, {}, R.SIZES_GRID, want_paths=[("sweep", 8)])


def test_instantiations_of_a_one_workgroup_grid(prob):
    """NSX_MGS_MAXWG=1: 8 entries per thread up to n = 2048, 10 up to 2560, 12 up to 3072, two passes beyond -- each at its last
    length and one more (a thread's tail entry, the first entry of the next instantiation)"""
    run_handle(prob, {"NSX_MGS_MAXWG": "1"}, R.SIZES_WG1,
               want_paths=[("sweep", 8), ("sweep", 10), ("sweep", 12), ("two_pass", None)])


def test_instantiations_of_a_three_workgroup_grid(prob):
    """NSX_MGS_MAXWG=3: three workgroups reduce up to 59 values (value v by workgroup v % 3) at 8, 10 and 12 entries per thread"""
    run_handle(prob, {"NSX_MGS_MAXWG": "3"}, R.SIZES_WG3,
               want_paths=[("sweep", 8), ("sweep", 10), ("sweep", 12)])


def test_two_pass_sweep(prob):
    """k_ls_dots / k_ls_finalize / k_ls_solve / k_ls_update on vectors too long for a one-workgroup grid: up to 293 workgroups of the
    dot kernel (more partial sums per value than k_ls_finalize has threads), every dim through the LS_C = 8 passes, all three guards"""
    run_handle(prob, {"NSX_MGS_MAXWG": "1"}, (3073, 5000, 100001, 300001), want_paths=[("two_pass", None)])


COMM_SIZES = R.SIZES_GRID


@pytest.mark.parametrize("n", COMM_SIZES)
def test_collective_inside_the_grid(prob, n):
    """k_mgs_one<8,10,true> on a 1-rank RCCL communicator (one handle per length: the ranks agree once per handle whether a vector's role
    fits the resident grid)"""
    run_handle(prob, {}, (n,), comm=True, want_paths=[("sweep", 8)])


@pytest.mark.parametrize("n", COMM_SIZES)
def test_two_passes_with_a_communicator(prob, n):
    run_handle(prob, {"NSX_MGS_DIST": "0"}, (n,), comm=True, want_paths=[("two_pass", None)])


@pytest.mark.parametrize("n", COMM_SIZES)
def test_chain_with_a_communicator(prob, n):
    run_handle(prob, {"NSX_MGS_DIST": "0", "NSX_MGS_LOWSYNC": "0"}, (n,), comm=True, want_paths=[("chain", None)])
