"""Extended-precision reference of the Krylov drivers' BLAS-1 layer (csrc/nsx_blas.hip, k_reciprocal of csrc/nsx_solve.hip), the derived
bounds it is compared under, and a float64 model of the kernels with mutants (tests/test_gpu_blas1.py runs the comparison on the device
through the hook nsx_blas1_run; tests/test_blas_reference.py shows on the CPU that it rejects every mutant).  A plain helper module.

A PROGRAM is a list of dicts as Nsx.blas1_run takes them ("kind" of nsx.BLAS1_KINDS and the fields of nsx_blas1_op).  Vectors are
rows of W[m][n + gap] in the device layout of a Span(n, split, gap): logical entry i at i + (i >= split ? gap : 0).  An op with a
field "n" runs on the first n <= split entries alone (a plain length); the ops without a span (PLAIN) need that or gap == 0.

`compare` checks ONE op at a time, in np.longdouble, from the inputs the device itself had: the caller's vectors for a vector no op
has written yet, the downloaded vectors for one an earlier op wrote.  A program under comparison is therefore single-assignment --
every vector is written by at most one op (asserted) -- and no error of one op is charged to the next.  Bounds, with eps = 2^-52
(twice the unit round-off, which leaves room for the second-order terms and holds with or without FMA contraction):

  element-wise   d = s d + a v (k_axpby, the update halves of k_reduce<OP_ADD_AND_DOT> and k_cg_update; also d *= f, d = a / v):
                 entry by entry  2 eps (|s d| + |a v|)
  multi-axpy     x = x0 + sum_j c_j v_j [then -y + x]:  (k + 1) eps (|x0| + |y| + sum_j |c_j v_j|); two launches above 32 terms
                 round no more often than one chain of k links
  reductions     (depth + 1) eps sum_i |a_i b_i|, depth = the longest chain of additions behind the value, read from the code:
                   ceil(n / (256 nb))   terms a thread accumulates (nb workgroups of 256 threads, grid-stride)
                   + 6 + 4              block_sum_256: the wave's shuffle tree, then the four waves' sums one after the other
                   + 3 + 6  if nb > 1   slot_value: eight loads combined as a tree of depth 3, then the wave butterfly
                 (+ 1: the rounding of a_i b_i).  nb = red_blocks(n): min(512, ceil(n / 1024)), or 256 with a communicator.
                 The inputs are the DEVICE's vectors (for add_and_dot / cg_update the updated d / g as downloaded).
  device coefficient   c * value(num) / value(den): the slot values are taken as the device publishes them (the same slot_value
                 the consumer ran, bit for bit; tests/test_gpu_blas1.py asserts that bitwise on runs that differ only in where they
                 publish), multiplied and divided in float64 in the kernel's order -- no additions, so the coefficient is the
                 consumer's own, bit for bit -- and the expected vector is formed from it in extended precision.  The element bound
                 stays the derived one.
  published value      against the extended-precision sum of the reduction's inputs, under the reduction's bound.

Every comparison also requires: gap entries bitwise untouched, vectors no op writes bitwise untouched, every published value finite.

`model` is the float64 restatement: the kernels' own structure (per-workgroup partial sums in a slot's row, slot_nb, consumers that sum
the partial sums, finalisation and publication) with numpy's sums inside a workgroup.  MUTANTS are wrong versions of it."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended-precision long double (x87: eps 1.08e-19)"
EPS = float(np.finfo(np.float64).eps)

RED_BLOCKS, DIST_RED_BLOCKS, RED_STRIDE, MULTI_MAX, N_SLOTS = 512, 256, 1024, 32, 128
NAN_PAYLOAD = np.uint64(0x7FF80000DEADBEEF)          # the gap's filling: a quiet NaN that says where it came from
GAP_NAN = np.array([NAN_PAYLOAD], dtype=np.uint64).view(np.float64)[0]

REDUCTIONS = ("dot", "add_and_dot", "cg_update")
PLAIN = ("scale_vec", "cg_update", "cg_direction", "reciprocal")     # ops with a plain length: no span
MUTANTS = ("last_partial_dropped", "gap_ignored", "gap_entry_summed", "stale_slot", "denominator_ignored", "multi_above_32_dropped",
           "y_not_negated")


def cdiv(a, b):
    return -(-a // b)


def red_blocks(n, comm):
    return DIST_RED_BLOCKS if comm else max(1, min(RED_BLOCKS, cdiv(n, 1024)))


def ew_blocks(n):
    return max(1, min(2048, cdiv(n, 512)))


def depth(n, nb):
    return cdiv(n, 256 * nb) + 6 + 4 + (3 + 6 if nb > 1 else 0)


def index(n, split, gap):
    i = np.arange(n)
    return i + (i >= split) * gap


def to_layout(V, split, gap):
    """logical vectors V[m][n] -> storage W[m][n + gap], the gap filled with GAP_NAN"""
    V = np.asarray(V, dtype=np.float64)
    m, n = V.shape
    W = np.full((m, n + gap), GAP_NAN)
    W[:, index(n, split, gap)] = V
    return W


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return bool(np.array_equal(bits(a), bits(b)))


def writes(op):
    """rows of W an op writes"""
    k = op["kind"]
    if k in ("dot", "finalize", "read", "write_scalar"):
        return ()
    return (op["d"], op["w"]) if k == "cg_update" else (op["d"],)


def coefficient(c, num, den):
    """sval: c * value(num) / value(den) in float64, in the kernel's order (None = no slot)"""
    v = np.float64(c)
    if num is not None:
        v = v * np.float64(num)
    if den is not None:
        v = v / np.float64(den)
    return v


# ------------------------------------------------------------------------------------------------------------------ the comparison
def compare(ops, W0, Wd, out, scalars, split, gap, comm=False, slot_values=None):
    """(failures, {kernel: largest error / bound}).  W0: the vectors as uploaded, Wd / out / scalars: what the hook returned.
    slot_values {r: value}: what the device published for the result of the r-th reduction of the program (counting dot, add_and_dot
    and cg_update ops from 0) where THIS program leaves it unpublished: taken from a run of the same ops that publishes it."""
    W0, Wd = np.asarray(W0, dtype=np.float64), np.asarray(Wd, dtype=np.float64)
    m, n_span = W0.shape[0], W0.shape[1] - gap
    n, ix = n_span, index(n_span, split, gap)          # of the current op: its own length where it has one
    slot_values = slot_values or {}
    fails, ratios = [], {}
    cur = W0.copy()
    written, known, checked_ref = set(), {}, {}
    may_change = np.zeros(W0.shape, dtype=bool)          # storage entries some op may write
    n_sc, seen_reductions = 0, []

    def note(kernel, err, bound, tag):
        err, bound = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(bound, dtype=LD))
        if not np.all(np.isfinite(err)):
            fails.append("%s: not finite" % tag)
            return
        bad = np.flatnonzero((bound == 0) & (err != 0))
        r = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
        if len(bad):
            r = float("inf")
        ratios[kernel] = max(ratios.get(kernel, 0.0), r)
        if r > 1.0:
            worst = int(bad[0]) if len(bad) else int(np.argmax(err / np.where(bound > 0, bound, 1)))
            fails.append("%s: error / bound = %.3g at entry %d" % (tag, r, worst))

    def lg(row):
        return cur[row][ix].astype(LD)

    def value(slot, tag):
        assert slot in known and known[slot] is not None, "%s: the device's value of slot %d is not known to the comparison" % (tag, slot)
        return known[slot]

    def elementwise(kernel, tag, row, sv, av, vrow):
        d, s, a = lg(row), LD(sv), LD(av)
        v = lg(vrow) if vrow is not None else np.zeros(n, dtype=LD)
        note(kernel, np.abs(Wd[row][ix].astype(LD) - (s * d + a * v)), 2 * EPS * (np.abs(s * d) + np.abs(a * v)), tag)

    def reduction(kernel, tag, i, a, b, slot):
        nb = red_blocks(n, comm)
        ref, scale = np.sum(a * b), np.sum(np.abs(a * b))
        checked_ref[slot] = (ref, (depth(n, nb) + 1) * EPS * scale, kernel, tag)
        if ops[i].get("read"):
            known[slot] = np.float64(out[i])
        elif len(seen_reductions) in slot_values:
            known[slot] = np.float64(slot_values[len(seen_reductions)])
        else:
            known[slot] = None
        seen_reductions.append(i)
        if known[slot] is not None:
            published(slot, known[slot])

    def published(slot, val):
        if not np.isfinite(val):
            fails.append("slot %d: published value %r" % (slot, val))
        elif slot in checked_ref:
            ref, bound, kernel, tag = checked_ref[slot]
            note(kernel, abs(LD(val) - ref), bound, tag + " (value)")

    for i, op in enumerate(ops):
        kind = op["kind"]
        tag = "op %d %s" % (i, kind)
        n = op.get("n", 0) or n_span
        assert n == n_span or n <= split
        ix = index(n, split, gap) if n == n_span else np.arange(n)
        assert gap == 0 or n < n_span or kind not in PLAIN, "%s takes a plain length" % tag
        for row in writes(op):
            assert row not in written, "%s: vector %d is written twice (the comparison needs single-assignment programs)" % (tag, row)
        if kind == "dot":
            reduction("k_reduce<OP_DOT>", tag, i, lg(op["d"]), lg(op["w"]), op["slot"])
        elif kind == "add_and_dot":
            al = coefficient(op.get("a", 0.0), value(op["num"], tag) if op.get("num", -1) >= 0 else None, None)
            elementwise("k_reduce<OP_ADD_AND_DOT>", tag, op["d"], 1.0, al, op["v"])
            dnew = Wd[op["d"]][ix].astype(LD)
            reduction("k_reduce<OP_ADD_AND_DOT>", tag, i, dnew, dnew if op["w"] == op["d"] else lg(op["w"]), op["slot"])
        elif kind in ("add", "add_dev", "sadd", "scale", "scale_dev_inv", "cg_direction"):
            sv, av, vrow = 1.0, 0.0, op.get("v")
            if kind == "add":
                av = np.float64(op["a"])
            elif kind == "add_dev":
                av = coefficient(op["a"], value(op["num"], tag), None)
            elif kind == "sadd":
                sv, av = np.float64(op["s"]), np.float64(op["a"])
            elif kind == "scale":
                sv, vrow = np.float64(op["a"]), None
            elif kind == "scale_dev_inv":
                sv, vrow = coefficient(1.0, None, value(op["den"], tag)), None
            else:
                sv, av = coefficient(1.0, value(op["num"], tag), value(op["den"], tag)), -1.0
            elementwise("k_axpby", tag, op["d"], sv, av, vrow)
        elif kind == "scale_vec":
            p = lg(op["d"]) * lg(op["v"])
            note("k_scale_vec", np.abs(Wd[op["d"]][ix].astype(LD) - p), 2 * EPS * np.abs(p), tag)
        elif kind == "reciprocal":
            q = LD(op["a"]) / lg(op["v"])
            note("k_reciprocal", np.abs(Wd[op["d"]][ix].astype(LD) - q), 2 * EPS * np.abs(q), tag)
        elif kind in ("axpy_multi", "axpy_multi_into"):
            k = len(op.get("vs", ()))
            x0 = lg(op["d"]) if kind == "axpy_multi" else (lg(op["v"]) if op.get("v", -1) >= 0 else np.zeros(n, dtype=LD))
            y = lg(op["w"]) if kind == "axpy_multi_into" and op.get("w", -1) >= 0 else None
            s, mag = x0.copy(), np.abs(x0)
            for j, c in zip(op.get("vs", ()), op.get("coef", ())):
                assert j not in writes(op)
                t = LD(np.float64(c)) * lg(j)
                s, mag = s + t, mag + np.abs(t)
            if y is not None:
                s, mag = s - y, mag + np.abs(y)
            kernel = "k_axpy_multi" if kind == "axpy_multi" else "k_axpy_multi_from" if op.get("v", -1) >= 0 else "k_axpy_multi_zero"
            note(kernel, np.abs(Wd[op["d"]][ix].astype(LD) - s), (k + 1) * EPS * mag, tag)
        elif kind == "cg_update":
            al = coefficient(1.0, value(op["num"], tag), value(op["den"], tag))
            elementwise("k_cg_update", tag + " x", op["d"], 1.0, al, op["v"])
            elementwise("k_cg_update", tag + " g", op["w"], 1.0, al, op["x"])
            g = Wd[op["w"]][ix].astype(LD)
            reduction("k_cg_update", tag, i, g, g, op["slot"])
        elif kind == "finalize":
            pass
        elif kind == "read":
            vals = scalars[n_sc:n_sc + op["count"]]
            n_sc += op["count"]
            if out[i] != vals[0] and not (np.isnan(out[i]) and np.isnan(vals[0])):
                fails.append("%s: out %r is not the first value %r" % (tag, out[i], vals[0]))
            for s, v in zip(range(op["slot"], op["slot"] + op["count"]), vals):
                if known.get(s) is not None:
                    if not same_bits(known[s], v):
                        fails.append("%s: slot %d reads %r, the device had published %r" % (tag, s, v, known[s]))
                elif s in checked_ref or s in known:
                    known[s] = np.float64(v)
                    published(s, known[s])
        elif kind == "write_scalar":
            known[op["slot"]] = np.float64(op["a"])
            checked_ref.pop(op["slot"], None)
            if op.get("read") and not same_bits(out[i], op["a"]):
                fails.append("%s: reads %r" % (tag, out[i]))
        else:
            raise ValueError(kind)
        for row in writes(op):
            written.add(row)
            cur[row] = Wd[row]
            may_change[row][ix] = True
    for row in range(m):
        keep = ~may_change[row]
        if not same_bits(Wd[row][keep], W0[row][keep]):
            fails.append("vector %d: entries no op may write were changed (the gap, the tail behind an op's own length, an untouched vector)" % row)
    return fails, ratios


# ------------------------------------------------------------------------------------------------------------------ the float64 model
def model(ops, W0, split, gap, comm=False, mutant=None):
    """what the kernels compute, restated in float64 on the storage layout: (vectors afterwards, out, scalars).  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    W = np.array(W0, dtype=np.float64, copy=True)
    m, n_span = W.shape[0], W.shape[1] - gap
    scal, partial, slot_nb = np.zeros(N_SLOTS), np.zeros((N_SLOTS, RED_STRIDE)), np.zeros(N_SLOTS, dtype=int)
    out, scalars = np.zeros(len(ops)), []

    def slot_value(slot):
        nb = slot_nb[slot]
        if nb == 0:
            return scal[slot]
        return np.sum(partial[slot][:nb - 1 if mutant == "last_partial_dropped" else nb])

    def sval(c, num, den):
        return coefficient(c, slot_value(num) if num >= 0 else None, slot_value(den) if den >= 0 and mutant != "denominator_ignored" else None)

    def reduce_into(slot, prod):
        n = len(prod)
        nb = red_blocks(n, comm)
        pad = np.zeros(cdiv(n, 256 * nb) * 256 * nb)
        pad[:n] = prod
        sums = pad.reshape(-1, nb, 256).sum(axis=(0, 2))   # workgroup b takes entries b * 256 + t + k * (256 nb)
        if mutant == "gap_entry_summed" and gap > 0 and n == n_span:
            sums[-1] += W[0][split]
        if nb > 1:
            partial[slot][:nb] = sums
            slot_nb[slot] = nb
        else:
            scal[slot] = sums[0]
            if mutant != "stale_slot":
                slot_nb[slot] = 0

    def publish(slot):
        scal[slot] = slot_value(slot)
        slot_nb[slot] = 0
        return scal[slot]

    for i, op in enumerate(ops):
        kind = op["kind"]
        g = lambda key: op.get(key, -1)   # noqa: E731
        n = op.get("n", 0) or n_span
        ix = np.arange(n) if mutant == "gap_ignored" or n < n_span else index(n, split, gap)
        if kind == "dot":
            reduce_into(op["slot"], W[op["d"]][ix] * W[op["w"]][ix])
        elif kind == "add_and_dot":
            W[op["d"]][ix] += sval(op.get("a", 0.0), g("num"), -1) * W[op["v"]][ix]
            reduce_into(op["slot"], W[op["d"]][ix] * W[op["w"]][ix])
        elif kind == "add":
            W[op["d"]][ix] = 1.0 * W[op["d"]][ix] + np.float64(op["a"]) * W[op["v"]][ix]
        elif kind == "add_dev":
            W[op["d"]][ix] = 1.0 * W[op["d"]][ix] + sval(op["a"], op["num"], -1) * W[op["v"]][ix]
        elif kind == "sadd":
            W[op["d"]][ix] = np.float64(op["s"]) * W[op["d"]][ix] + np.float64(op["a"]) * W[op["v"]][ix]
        elif kind == "scale":
            W[op["d"]][ix] = np.float64(op["a"]) * W[op["d"]][ix]
        elif kind == "scale_dev_inv":
            W[op["d"]][ix] = sval(1.0, -1, op["den"]) * W[op["d"]][ix]
        elif kind == "cg_direction":
            W[op["d"]][:n] = sval(1.0, op["num"], op["den"]) * W[op["d"]][:n] - W[op["v"]][:n]
        elif kind == "scale_vec":
            W[op["d"]][:n] *= W[op["v"]][:n]
        elif kind == "reciprocal":
            W[op["d"]][:n] = np.float64(op["a"]) / W[op["v"]][:n]
        elif kind in ("axpy_multi", "axpy_multi_into"):
            vs, coef = list(op.get("vs", ())), list(op.get("coef", ()))
            if kind == "axpy_multi_into":
                assert len(vs) <= MULTI_MAX and not (g("v") >= 0 and g("w") >= 0)
                s = W[op["v"]][ix].copy() if g("v") >= 0 else np.zeros(n)
            else:
                s = W[op["d"]][ix].copy()
                if mutant == "multi_above_32_dropped":
                    vs, coef = vs[:MULTI_MAX], coef[:MULTI_MAX]
            for j, c in zip(vs, coef):
                s += np.float64(c) * W[j][ix]
            if kind == "axpy_multi_into" and g("w") >= 0:
                s = (W[op["w"]][ix] if mutant == "y_not_negated" else -W[op["w"]][ix]) + s
            if kind == "axpy_multi_into" or len(vs):
                W[op["d"]][ix] = s
        elif kind == "cg_update":
            al = sval(1.0, op["num"], op["den"])
            W[op["d"]][:n] += al * W[op["v"]][:n]
            W[op["w"]][:n] += al * W[op["x"]][:n]
            reduce_into(op["slot"], W[op["w"]][:n] ** 2)
        elif kind == "finalize":
            assert op["count"] <= 64
            for s in range(op["slot"], op["slot"] + op["count"]):
                publish(s)
        elif kind == "read":
            assert op["count"] <= 64
            vals = [publish(s) for s in range(op["slot"], op["slot"] + op["count"])]
            scalars += vals
            out[i] = vals[0]
        elif kind == "write_scalar":
            scal[op["slot"]] = op["a"]
            if mutant != "stale_slot":
                slot_nb[op["slot"]] = 0
        else:
            raise ValueError(kind)
        if op.get("read") and kind != "read":
            out[i] = publish(op["slot"])
    return W, out, np.array(scalars)


# ------------------------------------------------------------------------------------------------------------------ the cases
SEED = 414
SIZES = (1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 64 * 1024 + 1, 511 * 1024 + 1, 512 * 1024, 512 * 1024 + 257)
SIZES_COMM = (1, 257, 256 * 256 + 1, 256 * 1024 + 1)
KS = (0, 1, 28, 32, 33, 40)
A, B, C_ = 50, 51, 52          # three of the solvers' slots (inside S_H2's range: free between solves)


def spans(n):
    """(split, gap) of the issue's list that exist at this length, without duplicates"""
    cand = [(n, 0), (0, 7), (1, 7), (256, 512), (300, 7), (1024, 1), (n - 1, 7)]
    seen, res = set(), []
    for s, g in cand:
        if 0 <= s <= n and (s < n or g == 0) and (s, g) not in seen:
            seen.add((s, g))
            res.append((s, g))
    return res


def gauss(m, n, seed=SEED):
    return np.random.default_rng([seed, m, n]).standard_normal((m, n))


def cancelling(n, seed=SEED):
    """(a, b) with a . b about 1e-12 of sum |a_i b_i| (n >= 2): b's component along a is taken out in extended precision, then put back
    at that size"""
    a, b = gauss(2, n, seed + 1)
    al, bl = a.astype(LD), b.astype(LD)
    scale = np.sum(np.abs(al * bl))
    b = (bl - (np.sum(al * bl) - LD(1e-12) * scale) / np.sum(al * al) * al).astype(np.float64)
    return a, b


def span_program(k_multi=3):
    """every spanned op once, single-assignment, on 12 + k_multi vectors: rows 0..3 are read only; the slots A, B stay in partial sums
    where the length gives more than one workgroup, and are consumed that way"""
    base = 12
    vs = list(range(base, base + k_multi))
    coef = [(-1) ** j * (0.5 + 0.1 * j) for j in range(k_multi)]
    return [
        dict(kind="dot", d=0, w=1, slot=A),
        dict(kind="dot", d=1, w=1, slot=B),
        dict(kind="add_dev", d=4, a=0.75, num=A, v=2),
        dict(kind="scale_dev_inv", d=5, den=B),
        dict(kind="add_and_dot", d=6, a=-1.25, num=A, v=3, w=0, slot=C_),
        dict(kind="add_and_dot", d=7, a=0.5, num=C_, v=3, w=7, slot=C_ + 1, read=1),
        dict(kind="add", d=8, a=-0.3, v=2),
        dict(kind="sadd", d=9, s=1.7, a=0.9, v=3),
        dict(kind="scale", d=10, a=-2.5),
        dict(kind="axpy_multi", d=11, vs=vs, coef=coef),
        dict(kind="read", slot=A, count=3),
    ], base + k_multi


def published_twin(ops):
    """the same program with every reduction publishing its value at once: where the device's slot values come from"""
    return [dict(op, read=1) if op["kind"] in REDUCTIONS else op for op in ops]


def slot_values_from(ops, out):
    """{r: value} of the reductions a run published at once (compare's slot_values)"""
    red = [i for i, op in enumerate(ops) if op["kind"] in REDUCTIONS]
    return {r: out[i] for r, i in enumerate(red) if ops[i].get("read")}


def plain_program():
    """the ops with a plain length, single-assignment, on 12 vectors"""
    return [
        dict(kind="dot", d=0, w=1, slot=A),
        dict(kind="dot", d=1, w=1, slot=B),
        dict(kind="cg_direction", d=4, v=2, num=A, den=B),
        dict(kind="cg_update", d=5, v=2, w=6, x=3, num=A, den=B, slot=C_),
        dict(kind="cg_direction", d=7, v=3, num=C_, den=B),
        dict(kind="scale_vec", d=8, v=2),
        dict(kind="reciprocal", d=9, v=3, a=-1.0),
        dict(kind="read", slot=C_, count=1),
    ], 12


def chain_programs(spanned):
    """a dot into A and a dot into B, then consumers of c * A / B, with the two slots still in partial sums, both final, one of each, and
    published one by one: {name: program}.  The vectors that come back must be bitwise the same in all four.  spanned: consumers that
    take a span (add_dev with A, scale_dev_inv with B, add_and_dot with w != d and with the self branch w == d), else the plain-length
    ones (cg_direction, cg_update with A / B)."""
    dots = [dict(kind="dot", d=0, w=1, slot=A), dict(kind="dot", d=1, w=1, slot=B)]
    if spanned:
        use = [dict(kind="add_dev", d=4, a=0.75, num=A, v=2), dict(kind="scale_dev_inv", d=5, den=B),
               dict(kind="add_and_dot", d=6, a=-1.25, num=B, v=3, w=0, slot=C_),
               dict(kind="add_and_dot", d=7, a=0.5, num=A, v=3, w=7, slot=C_ + 1)]
    else:
        use = [dict(kind="cg_direction", d=4, v=2, num=A, den=B), dict(kind="cg_update", d=5, v=2, w=6, x=3, num=A, den=B, slot=C_)]
    tail = [dict(kind="read", slot=C_, count=2 if spanned else 1)]
    return {"partials": dots + use + tail,
            "final": dots + [dict(kind="finalize", slot=A, count=2)] + use + tail,
            "mixed": dots + [dict(kind="finalize", slot=B, count=1)] + use + tail,
            "published": published_twin(dots) + use + tail}, 8


def stale_programs(n_short):
    """a long dot leaves its partial sums in A; then A is rewritten by a dot over the first n_short <= 1024 entries (one workgroup: the
    value goes straight to the slot) or by write_scalar; the consumer must see the new value: {name: program}"""
    long_dot, use = dict(kind="dot", d=0, w=1, slot=A), dict(kind="add_dev", d=4, a=0.75, num=A, v=2)
    return {"short_dot": [long_dot, dict(kind="dot", d=2, w=3, slot=A, n=n_short), use],
            "write_scalar": [long_dot, dict(kind="write_scalar", slot=A, a=0.625), use]}, 5


READ_SLOT0, READ_COUNT = 8, 64


def read_range_program(n_short):
    """64 slots in a row, alternately left in partial sums by a dot over the whole span and final (a dot over n_short entries, every
    eighth one written from the host), published twice back to back (the counter of the publication's last block must have reset itself)"""
    ops = []
    for j in range(READ_COUNT):
        s = READ_SLOT0 + j
        if j % 8 == 7:
            ops.append(dict(kind="write_scalar", slot=s, a=float(j) + 0.5))
        elif j % 2:
            ops.append(dict(kind="dot", d=j % 4, w=(j // 4) % 4, slot=s, n=n_short))
        else:
            ops.append(dict(kind="dot", d=j % 4, w=(j // 4) % 4, slot=s))
    return ops + [dict(kind="read", slot=READ_SLOT0, count=READ_COUNT)] * 2, 4


def multi_programs(k):
    """the update of x by k vectors in its three forms on 4 + k vectors (row 0: x0, row 1: y, rows 2 and 3: results):
    {name: (program, row that holds the result)}"""
    vs = list(range(4, 4 + k))
    coef = [(-1) ** j * (0.25 + 0.05 * j) for j in range(k)]
    progs = {"self": ([dict(kind="axpy_multi", d=0, vs=vs, coef=coef)], 0)}
    if k <= MULTI_MAX:
        progs["from"] = ([dict(kind="axpy_multi_into", d=2, v=0, vs=vs, coef=coef)], 2)
        progs["zero"] = ([dict(kind="axpy_multi_into", d=2, vs=vs, coef=coef)], 2)
        progs["zero_y"] = ([dict(kind="axpy_multi_into", d=2, w=1, vs=vs, coef=coef)], 2)
        progs["zero_y_alias"] = ([dict(kind="axpy_multi_into", d=1, w=1, vs=vs, coef=coef)], 1)
        progs["zero_then_sadd"] = ([dict(kind="axpy_multi_into", d=2, vs=vs, coef=coef), dict(kind="sadd", d=1, s=-1.0, a=1.0, v=2)], 1)
    return progs, 4 + k
