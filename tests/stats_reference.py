"""A numpy restatement of the running statistics' contract (include/nsx.h, section "running statistics"), parametrised by dtype.

The float64 run does, operation by operation, what csrc/nsx_stats.hip does (numpy rounds every elementwise operation on its own and never
contracts a product and a sum): the device has to reproduce it bit for bit.  The np.longdouble run (64-bit mantissa on x86: LONG_OK) takes
the SAME double coefficients r, q, s, t -- they are part of the contract, formed on the host in double -- and is the extended-precision
reference the rounding bounds are measured against.  Pinned by tests/test_stats_reference.py."""
import numpy as np

U = 2.0 ** -53
LONG_OK = np.finfo(np.longdouble).nmant >= 63


def nsym(nc):
    return nc * (nc + 1) // 2


def pairs(nc):
    """(i, j), i <= j, in the order of the co-moment planes: xx, yy, [zz,] xy[, xz, yz]"""
    return [(i, i) for i in range(nc)] + sorted(((i, j) for i in range(nc) for j in range(i + 1, nc)), key=lambda p: p[0] + p[1])


def update_coefficients(W, w):
    """W' = W + w, r = w / W', q = W r: three doubles, one rounded operation each"""
    W, w = np.float64(W), np.float64(w)
    W1 = W + w
    r = w / W1
    return W1, r, W * r


def merge_coefficients(Wa, Wb):
    """W = W_a + W_b, s = W_b / W, t = W_a s"""
    Wa, Wb = np.float64(Wa), np.float64(Wb)
    W = Wa + Wb
    s = Wb / W
    return W, s, Wa * s


class Accumulator:
    """mean m [n][nc] and co-moment C [n][nsym(nc)] of one bin in `dtype`; W (a double) and the sample count as the handle keeps them"""

    def __init__(self, n, nc, dtype=np.float64):
        self.nc, self.dtype = nc, dtype
        self.m, self.C = np.zeros((n, nc), dtype), np.zeros((n, nsym(nc)), dtype)
        self.W, self.samples = np.float64(0.0), 0

    def add(self, x, w):
        x = np.asarray(x, dtype=np.float64).reshape(self.m.shape).astype(self.dtype)
        W1, r, q = update_coefficients(self.W, w)
        r, q = self.dtype(r), self.dtype(q)
        d = x - self.m
        self.m = self.m + r * d
        for k, (i, j) in enumerate(pairs(self.nc)):
            self.C[:, k] = self.C[:, k] + (q * d[:, i]) * d[:, j]
        self.W, self.samples = W1, self.samples + 1
        return self

    def merged(self, b):
        """the pairwise merge (self, b) -> a new accumulator; neither operand changes"""
        a = self
        out = Accumulator(len(a.m), a.nc, a.dtype)
        W, s, t = merge_coefficients(a.W, b.W)
        s, t = a.dtype(s), a.dtype(t)
        delta = b.m - a.m
        for k, (i, j) in enumerate(pairs(a.nc)):
            out.C[:, k] = (a.C[:, k] + b.C[:, k]) + (t * delta[:, i]) * delta[:, j]
        out.m = a.m + s * delta
        out.W, out.samples = W, a.samples + b.samples
        return out


def pooled(bins):
    """the non-empty bins folded in ascending order; None when all are empty"""
    acc = None
    for b in bins:
        if b.samples == 0:
            continue
        acc = b if acc is None else acc.merged(b)
    return acc


def derive(m, C, W, dtype=np.float64):
    """the derived quantities from raw planes m [n][nc], C [n][nsym] and the bin's weight W (a double), every operation in `dtype`:
    stress = C invW, rms = sqrt(C_ii invW), tke = (R_00 + R_11 [+ R_22]) / 2 summed left to right (nc = 1: variance and rms of the pressure)"""
    m, C = np.asarray(m).astype(dtype), np.asarray(C).astype(dtype)
    nc = m.shape[1]
    invW = dtype(1.0) / dtype(W)
    stress = C * invW
    rms = np.sqrt(stress[:, :nc])
    e = stress[:, 0].copy()
    for c in range(1, nc):
        e = e + stress[:, c]
    return {"stress": stress, "rms": rms, "tke": (dtype(0.5) * e).reshape(-1, 1)}


def two_pass(xs, ws):
    """weighted mean and co-moment sum_k w_k (x_k - mean)_i (x_k - mean)_j of the samples xs [n_samples][n][nc] in long double, two passes"""
    xs = np.asarray(xs, dtype=np.float64).astype(np.longdouble)
    ws = np.asarray(ws, dtype=np.float64).astype(np.longdouble)
    W = ws.sum()
    mean = (ws[:, None, None] * xs).sum(axis=0) / W
    d = xs - mean
    nc = xs.shape[2]
    C = np.stack([(ws[:, None] * d[:, :, i] * d[:, :, j]).sum(axis=0) for i, j in pairs(nc)], axis=1)
    return mean, C, W


def bounds(xs, ws):
    """the rounding bounds of the float64 run against the long-double run (derived in tests/test_stats_reference.py): mean 5 n u X_i,
    co-moment (24 n + 16) u W X_i X_j with X_i = max_k |x_k,i| per DoF"""
    xs = np.asarray(xs, dtype=np.float64)
    n = len(xs)
    X = np.abs(xs).max(axis=0).astype(np.longdouble)
    W = np.asarray(ws, dtype=np.float64).astype(np.longdouble).sum()
    nc = xs.shape[2]
    bm = 5 * n * U * X
    bC = np.stack([(24 * n + 16) * U * W * X[:, i] * X[:, j] for i, j in pairs(nc)], axis=1)
    return bm, bC


def ratio(got, ref, bound):
    """largest |got - ref| / bound (0 / 0 = 0: where the bound vanishes the values have to agree exactly)"""
    d = np.abs(np.asarray(got).astype(np.longdouble) - np.asarray(ref).astype(np.longdouble))
    b = np.asarray(bound, dtype=np.longdouble)
    if d.size == 0:
        return 0.0
    return float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1), np.where(d == 0, 0.0, np.inf))))


def run(xs, ws, bins=None, n_bins=1, dtype=np.float64):
    """feed the samples xs [n_samples][n][nc] with weights ws into n_bins accumulators (bins[k]: the bin of sample k, default 0)"""
    xs = np.asarray(xs, dtype=np.float64)
    accs = [Accumulator(xs.shape[1], xs.shape[2], dtype) for _ in range(n_bins)]
    for k, (x, w) in enumerate(zip(xs, ws)):
        accs[0 if bins is None else bins[k]].add(x, w)
    return accs
