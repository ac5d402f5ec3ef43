"""Extended-precision reference of one Gram-Schmidt cycle of the sweep kernels (csrc/nsx_mgs.hip), the yardstick it is measured with,
and the comparison the GPU tests call (tests/test_gpu_mgs_sweep.py; checked on the CPU by tests/test_mgs_reference.py).  A plain
helper module, no fixtures.

The cycle is the one nsx_gram_schmidt_sweeps runs: vector 0 is normalised; vector k goes through deal.II's modified Gram-Schmidt chain
against the k vectors in front of it -- h_i = w . v_i, w -= h_i v_i for i ascending -- then |w|^2, then w / |w|.

* `reference(n, m, seed, kind)`: that chain in np.longdouble (x87 extended, eps 1.08e-19) with pairwise sums, on seeded float64 input,
  AND the same chain in float64.  The deviation of the float64 chain from the extended one -- `err64` per quantity -- is the yardstick:
  it is what a correct implementation in the kernels' own number format loses on this very input.
* `compare(...)`: every quantity a cycle returns against the reference, each with the bound  K * (err64 + FLOOR)  (FLOOR = 4 eps: a
  quantity the float64 chain happens to hit exactly must not make the bound vanish).  K is the margin for another, equally valid
  grouping of the sums (per thread, wave, workgroup, grid; the Gram-matrix evaluation of the coefficients): measured on the MI355X,
  10 x the largest ratio seen, rounded up -- see K below.

Scales (what "relative" means per quantity):
  Q     entry by entry, relative to max |Q_k| of the reference vector
  H     h_ki relative to |w_k| before the sweep (a dot product of w with a unit vector carries an absolute error of eps |w|, whatever
        the size of the coefficient itself)
  orth  max |Q Q^T - I| of the vectors as they came back, absolute (the float64 chain's own loss of orthogonality is its err64)
  |w'|^2 after the sweep, |w|^2 before it: relative to themselves.  Where the variant takes |w'|^2 from the Gram formula
        |w|^2 - 2 h.r + h^T G h the kernel's documented error model  eps * dim * |w|^2 / |w'|^2  (nsx_mgs.hip, above mgs_norm_guard) is
        added to err64 + FLOOR, from the reference's numbers.
A vector the sweep all but annihilates (kind "dependent": 1e-9 of its norm is left) is what remains of a cancellation by nine digits:
its direction and |w'|^2 are determined to eps |w| / |w'| = 1e-7 only, in ANY float64 implementation.  For that vector Q_k |w'| (the
unnormalised remainder) and |w'| are compared relative to max |w_k| and |w_k| before the sweep -- the scale their errors have -- with
the same K and the float64 chain's deviation on that scale; every bound stays below 1e-10 (asserted in compare)."""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended-precision long double (x87: eps 1.08e-19)"
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS

# Margin over the float64 chain's own deviation.  Largest ratios  error / (err64 + FLOOR [+ Gram model])  measured on the MI355X
# over every variant x instantiation x size x span x flag of tests/test_gpu_mgs_sweep.py (recorded as "mgs_sweep_unit"):
#   Q 0.55, H 0.16, |w'|^2 0.34, |w|^2 before 0.25, max |Q Q^T - I| 0.72 (two passes at n = 600001; one exchange 0.69, chain 0.65),
#   the annihilated vector: remainder 0.45, |w'| 0.09
# -- every variant stays INSIDE the float64 chain's own deviation + 4 eps (fixed-order tree sums lose less than the chain's).
# K = 10 x the largest of them (0.72), rounded up.
K = 8.0
HARD_LIMIT = 1e-10  # no asserted bound may reach this (relative, on the scales above)

KINDS = ("gauss", "dependent")
SEED = 2024
# vector lengths of tests/test_gpu_mgs_sweep.py: the real grid (one entry up to more than 256 workgroups), and the edges of the
# instantiations mgs_pick chooses for a grid capped at one workgroup (8 / 10 / 12 entries per thread,
# two passes beyond) and at three
SIZES_GRID = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000, 100001, 300001, 600001)
SIZES_WG1 = (2047, 2048, 2049, 2560, 2561, 3072, 3073)
SIZES_WG3 = (6144, 6145, 7681)
ALL_SIZES = tuple(sorted(set(SIZES_GRID + SIZES_WG1 + SIZES_WG3)))


def spans(n):
    """(split, gap) of the block-vector layouts a length is tested in; None = contiguous"""
    return [None] + sorted({(n // 3, 37), (0, 5), (n - 1, 1)})


def make_vectors(n, m, seed, kind="gauss"):
    """m seeded standard-normal vectors of length n (float64).  kind "dependent": the LAST one is rebuilt as a combination of the
    others plus a remainder sized so that the sweep leaves 1e-9 of its norm."""
    rng = np.random.default_rng([seed, n, m])
    V = rng.standard_normal((m, n))
    if kind == "dependent":
        assert m >= 3 and n >= 2 * m
        c = rng.uniform(0.5, 1.5, m - 1)
        lead = c @ V[:m - 1]
        V[m - 1] = lead + (1e-9 * np.linalg.norm(lead) / np.linalg.norm(V[m - 1])) * V[m - 1]
    elif kind != "gauss":
        raise ValueError(kind)
    return V


def basis_length(n):
    """30 vectors where the length allows them to be well conditioned, otherwise n // 2 (at least one)"""
    return 30 if n >= 60 else max(1, n // 2)


def condition_number(V):
    s = np.linalg.svd(V, compute_uv=False)
    return float(s[0] / s[-1])


def _psum(x):
    return np.sum(x)  # numpy's pairwise summation: error ~ log2(n) eps instead of n eps


def chain(V, dtype, drop=None, stale=None, gram_short=False):
    """The cycle in `dtype`.  Returns Q [m][n], H [m][m], |w'|^2 [m], |w|^2 before each sweep [m] (entry 0: of vector 0 as it came).
    The keyword arguments restate a sweep WRONGLY (tests/test_mgs_reference.py: the comparison must notice each of them):
    drop = entry left out of every sum over the vector; stale = entry of w that no update w -= h v touches; gram_short = |w'|^2 from
    the Gram formula with the newest row of the Gram matrix summed one column short (its diagonal is missing)."""
    m, n = V.shape
    V = V.astype(dtype)
    Q, H = np.zeros((m, n), dtype), np.zeros((m, m), dtype)
    after, before, G = np.zeros(m, dtype), np.zeros(m, dtype), np.zeros((m, m), dtype)

    def dot(a, b):
        s = _psum(a * b)
        return s if drop is None else s - a[drop] * b[drop]

    before[0] = after[0] = dot(V[0], V[0])
    Q[0] = V[0] / np.sqrt(after[0])
    for k in range(1, m):
        w = V[k].copy()
        before[k] = dot(w, w)
        r = np.zeros(k, dtype)
        for i in range(k):
            H[k, i] = dot(w, Q[i])
            if gram_short:
                r[i] = dot(V[k], Q[i])
            keep = w[stale] if stale is not None else None
            w -= H[k, i] * Q[i]
            if stale is not None:
                w[stale] = keep
        after[k] = dot(w, w)
        if gram_short:  # |w|^2 - 2 h.r + h^T G h, G = Gram matrix of the basis; G[k-1][k-1] missing in THIS sweep
            for j in range(k - 1):  # the newest row (the older ones were summed by the earlier sweeps) ...
                G[k - 1, j] = G[j, k - 1] = dot(Q[k - 1], Q[j])
            G[k - 1, k - 1] = 0  # ... without its last column, the diagonal
            h = H[k, :k]
            after[k] = before[k] - 2 * (h @ r) + h @ (G[:k, :k] @ h)
            G[k - 1, k - 1] = dot(Q[k - 1], Q[k - 1])  # (the later sweeps find the row complete: ONE entry is missing per sweep)
        Q[k] = w / np.sqrt(after[k])
    return Q, H, after, before


class Reference:
    """Extended-precision result of one cycle, the float64 chain's deviation from it (err64) and the input it was computed from."""

    def __init__(self, n, m, seed, kind):
        self.n, self.m, self.kind = n, m, kind
        self.V = make_vectors(n, m, seed, kind)
        self.cond = condition_number(self.V[:m - 1] if kind == "dependent" else self.V)   # of the basis the sweeps run against
        self.Q, self.H, self.after, self.before = chain(self.V, LD)
        self.weak = {m - 1} if kind == "dependent" else set()   # vectors the sweep all but annihilates
        self.err64 = errors(self, *chain(self.V, np.float64))


@functools.lru_cache(maxsize=None)
def reference(n, m, seed, kind="gauss"):
    return Reference(n, m, seed, kind)


def errors(ref, Q, H, after, before, skip_before=False):
    """Largest deviation of a cycle's results from the reference, per quantity, on the scales of the module's docstring.
    "q_weak" / "after_weak": the remainder Q_k |w'| of the annihilated vectors entry by entry relative to max |w_k| before the sweep,
    and |w'| relative to |w_k|."""
    m = ref.m
    e = {"q": 0.0, "h": 0.0, "after": 0.0, "before": 0.0, "q_weak": 0.0, "after_weak": 0.0, "orth": 0.0}
    Q, H, after, before = (np.asarray(x, dtype=LD) for x in (Q, H, after, before))
    for k in range(m):
        w0 = np.sqrt(ref.before[k])
        if k in ref.weak:
            rest, rest_ref = Q[k] * np.sqrt(after[k]), ref.Q[k] * np.sqrt(ref.after[k])
            e["q_weak"] = max(e["q_weak"], float(np.max(np.abs(rest - rest_ref)) / np.max(np.abs(ref.V[k]))))
            e["after_weak"] = max(e["after_weak"], float(abs(np.sqrt(after[k]) - np.sqrt(ref.after[k])) / w0))
        else:
            e["q"] = max(e["q"], float(np.max(np.abs(Q[k] - ref.Q[k])) / np.max(np.abs(ref.Q[k]))))
            e["after"] = max(e["after"], float(abs(after[k] - ref.after[k]) / ref.after[k]))
        if k:
            e["h"] = max(e["h"], float(np.max(np.abs(H[k, :k] - ref.H[k, :k])) / w0))
        if not skip_before:
            e["before"] = max(e["before"], float(abs(before[k] - ref.before[k]) / ref.before[k]))
    # orthonormality of what came back, in float64 as it came back (the annihilated vector is orthogonal to 1e-7 only after ONE
    # sweep, in any implementation: left out)
    good = [k for k in range(m) if k not in ref.weak]
    Qg = np.asarray(Q[good], dtype=np.float64)
    e["orth"] = float(np.max(np.abs(Qg @ Qg.T - np.eye(len(good)))))
    return e


def to_layout(V, split, gap, sentinel):
    """logical vectors [m][n] -> device layout of a Span(n, split, gap): [m][n + gap], the gap entries set to `sentinel`"""
    m, n = V.shape
    out = np.empty((m, n + gap))
    out[:, :split] = V[:, :split]
    out[:, split:split + gap] = sentinel
    out[:, split + gap:] = V[:, split:]
    return out


def from_layout(W, split, gap):
    return np.concatenate([W[:, :split], W[:, split + gap:]], axis=1), W[:, split:split + gap]


def gram_model(ref):
    """largest eps * dim * |w|^2 / |w'|^2 over the sweeps whose |w'|^2 is compared relative to itself"""
    return max([EPS * k * float(ref.before[k] / ref.after[k]) for k in range(1, ref.m) if k not in ref.weak] or [0.0])


def bounds(ref, formula, k_margin=None):
    """bound per quantity: K * (err64 + FLOOR), for |w'|^2 by the Gram formula + the kernel's error model"""
    k_margin = K if k_margin is None else k_margin
    b = {q: k_margin * (ref.err64[q] + FLOOR) for q in ref.err64}
    if formula:
        b["after"] = k_margin * (ref.err64["after"] + FLOOR + gram_model(ref))
    return b


def compare(ref, vectors, coeffs, after, before, normalized, split=None, gap=0, sentinel=None, consider=False, formula=False,
            expect_normalized=None, k_margin=None):
    """One cycle's results (device layout) against the reference.  Returns (failures, ratios): a list of messages, empty when every
    assertion holds, and error / (bound / K) per quantity, the number K is fixed from."""
    n, m = ref.n, ref.m
    split = n if split is None else split
    W = np.asarray(vectors)
    failures = []
    if W.shape != (m, n + gap):
        return ["vectors have shape %s, expected %s" % (W.shape, (m, n + gap))], {}
    Q, hole = from_layout(W, split, gap)
    if gap:
        want = np.full(hole.shape, sentinel)
        if not np.array_equal(hole.view(np.uint64), want.view(np.uint64)):
            failures.append("%d gap entries were overwritten" % int((hole.view(np.uint64) != want.view(np.uint64)).sum()))
    for name, x in (("vectors", Q), ("coeffs", coeffs), ("after", after)) + ((("before", before),) if consider else ()):
        if not np.all(np.isfinite(np.asarray(x, dtype=np.float64))):
            failures.append("%s not finite" % name)
    if np.any(np.asarray(after, dtype=np.float64) <= 0):
        failures.append("|w'|^2 not positive")
    if failures:
        return failures, {}
    err = errors(ref, Q, coeffs, after, before, skip_before=not consider)
    bnd = bounds(ref, formula, k_margin)
    k_used = K if k_margin is None else k_margin
    ratios = {}
    for q in err:
        assert bnd[q] < HARD_LIMIT, (q, bnd[q])   # the check itself: no bound may be this loose
        ratios[q] = err[q] / (bnd[q] / k_used)
        if not err[q] <= bnd[q]:
            failures.append("%s: error %.3e > bound %.3e (err64 %.3e)" % (q, err[q], bnd[q], ref.err64[q]))
    if expect_normalized is not None and list(np.asarray(normalized)) != list(expect_normalized):
        failures.append("normalized flags %s, expected %s" % (list(np.asarray(normalized)), list(expect_normalized)))
    return failures, ratios
