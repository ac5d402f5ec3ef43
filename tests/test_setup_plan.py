"""CPU suite: the set-up planners -- host/ilu_levels.hpp, host/spmv_plan.hpp, host/gather_map.hpp and the structural product of
host/graph.hpp -- through a stand-alone program, tests/setup_plan_check.cpp, built here with AddressSanitizer and UBSan.  Every expected
value is made again from its definition with numpy and scipy on the graphs of the test meshes."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import nodal_reference as NR
from conftest import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = [("box", 2, 18), ("box", 3, 108), ("cylinder", 3, 2832)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("setup_plan") / "setup_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "setup_plan_check.cpp")], check=True)
    return exe


def run(program, tmp_path, command, *arrays):
    """the program's head line (split) and its other lines as integer arrays"""
    path = tmp_path / "input.txt"
    with open(path, "w") as f:
        for a in arrays:
            f.write(" ".join(str(int(x)) for x in np.asarray(a).ravel()) + "\n")
    r = subprocess.run([program, command, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]      # a sanitizer report ends the program with a status of its own
    lines = r.stdout.split("\n")
    return lines[0].split(), [np.array(s.split(), dtype=np.int64) for s in lines[1:-1]]


class Graphs:
    """connectivity and graphs of one mesh, made with scipy from the cell loop: A = P2 x P2, G = P2 x P1, B = P1 x P2"""

    def __init__(self, kind, dim, n_cells):
        p = Problem(kind, dim, 1) if kind != "box" else Problem(kind, dim)
        d = p.dofs
        assert d.n_cells == n_cells
        self.dim, self.n_cells = dim, n_cells
        self.c2 = NR.cell_nodes(d)
        self.c1 = np.asarray(d.cell_dofs)[:, [(dim + 1) * v + dim for v in range(dim + 1)]] - d.n_u
        self.N2, self.NP = d.n_u // dim, d.n_p
        inc = lambda c, n: sp.csr_matrix((np.ones(c.size), (np.repeat(np.arange(n_cells), c.shape[1]), c.ravel())), shape=(n_cells, n))
        i2, i1 = inc(self.c2, self.N2), inc(self.c1, self.NP)
        self.A, self.G, self.B = (pattern(m) for m in (i2.T @ i2, i2.T @ i1, i1.T @ i2))


def pattern(m):
    m = sp.csr_matrix(m)
    m.sum_duplicates()
    m.sort_indices()
    return m


_graphs = {}


def graphs(mesh):
    if mesh not in _graphs:
        _graphs[mesh] = Graphs(*mesh)
    return _graphs[mesh]


# ---------------------------------------------------------------- levels
def expected_levels(g, bptr, backward):
    """(per block, the list of its levels' rows), level of every row -- from level[i] = 1 + max level[j] over the in-block j on one side of i"""
    lev = np.zeros(g.shape[0], dtype=int)
    blocks = []
    for r0, r1 in zip(bptr[:-1], bptr[1:]):
        for i in (range(r1 - 1, r0 - 1, -1) if backward else range(r0, r1)):
            cols = g.indices[g.indptr[i]:g.indptr[i + 1]]
            dep = cols[(cols > i) & (cols < r1)] if backward else cols[(cols < i) & (cols >= r0)]
            lev[i] = 1 + lev[dep].max() if len(dep) else 0
        rows = np.arange(r0, r1)
        blocks.append([rows[lev[rows] == l] for l in range(lev[rows].max() + 1 if r1 > r0 else 0)])
    return blocks


def check_levels(program, tmp_path, g, bptr):
    n, nb = g.shape[0], len(bptr) - 1
    bptr = np.asarray(bptr)
    head, out = run(program, tmp_path, "levels", [n, nb], g.indptr, g.indices, bptr)
    assert head[0] == "ok" and len(out) == 17
    max_rows, max_levels, in_block_nnz, max_block_nnz = (int(x) for x in head[1:])
    lists, (in_lo, in_hi, in_cptr, in_cpos, fac_order), merged = (out[0:3], out[3:6]), out[6:11], (out[11:14], out[14:17])
    # in-block range of every row: exactly the columns inside the row's block
    rows = np.repeat(np.arange(n), np.diff(g.indptr))
    blk = np.searchsorted(bptr, np.arange(n), side="right") - 1                 # the last block that begins at or in front of the row: not an empty one
    inside = (g.indices >= bptr[blk[rows]]) & (g.indices < bptr[blk[rows] + 1])
    count = np.bincount(rows[inside], minlength=n)
    for i in range(n):
        assert np.array_equal(np.arange(in_lo[i], in_hi[i]), np.flatnonzero(inside & (rows == i)))
    assert np.array_equal(in_cptr, np.concatenate([[0], np.cumsum(count)]))
    assert all(np.array_equal(in_cpos[in_cptr[i]:in_cptr[i + 1]], in_lo[i] + np.arange(count[i])) for i in range(n))
    per_block = np.array([count[bptr[b]:bptr[b + 1]].sum() for b in range(nb)], dtype=int)
    assert in_block_nnz == inside.sum() and max_block_nnz == (per_block.max() if nb else 0)
    assert np.array_equal(fac_order, np.argsort(-per_block, kind="stable"))
    assert max_rows == (np.diff(bptr).max() if nb else 0)
    deepest = 0
    diag = np.array([g.indptr[i] + np.searchsorted(g.indices[g.indptr[i]:g.indptr[i + 1]], i) for i in range(n)])
    for backward in (False, True):
        want = expected_levels(g, bptr, backward)
        lvl_ptr, lrows, blk_off = lists[backward]
        assert np.array_equal(blk_off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        flat = [r for w in want for r in w]
        assert lvl_ptr[0] == 0 and np.array_equal(np.diff(lvl_ptr), [len(r) for r in flat])
        assert np.array_equal(lrows, np.concatenate(flat) if flat else [])
        assert all(np.all(np.diff(r) > 0) for r in flat)                        # ascending inside a level
        deepest = max([deepest] + [len(w) for w in want])
        # merged: level l = the blocks' level-l rows one after the other, in block order
        mptr, mrows, mrec = merged[backward]
        assert len(mptr) == max_levels + 1 and mptr[0] == 0
        for l in range(max_levels):
            parts = [w[l] for w in want if len(w) > l]
            assert np.array_equal(mrows[mptr[l]:mptr[l + 1]], np.concatenate(parts) if parts else [])
        assert mptr[-1] == n == len(mrows)
        rec = mrec.reshape(-1, 4)
        d = diag[mrows]
        first, end = (d + 1, in_hi[mrows]) if backward else (in_lo[mrows], d)
        assert np.array_equal(rec, np.stack([mrows, first, end, d], axis=1))
    assert max_levels == deepest


def rank_table(n, nb):
    return np.linspace(0, n, nb + 1).astype(int)


@pytest.mark.parametrize("mesh", MESHES)
def test_levels_follow_the_recurrence_and_the_in_block_ranges_the_blocks(program, tmp_path, mesh):
    g = graphs(mesh).A
    n = g.shape[0]
    for nb in sorted({1, min(8, n), max(1, n // 85)}):
        check_levels(program, tmp_path, g, rank_table(n, nb))


def test_levels_of_empty_blocks_one_row_blocks_and_one_block(program, tmp_path):
    g = graphs(MESHES[0]).A
    n = g.shape[0]
    check_levels(program, tmp_path, g, [0, 0, 1, 7, 7, 7, n - 1, n, n])        # empty first, in the middle (twice) and last; one-row blocks
    check_levels(program, tmp_path, g, [0, n])
    check_levels(program, tmp_path, g, np.arange(n + 1))                        # every block one row: one level each
    S = pattern(graphs(MESHES[0]).B @ graphs(MESHES[0]).B.T)                   # the Schur graph: the second schedule of a handle
    check_levels(program, tmp_path, S, [0, 5, 5, S.shape[0]])


# ---------------------------------------------------------------- chunk bounds
def bounds(program, tmp_path, n, rk, target, allowed=True):
    head, out = run(program, tmp_path, "bounds", [n, target, int(allowed), len(rk)], rk)
    assert head == ["ok"]
    b = out[0]
    assert b[0] == 0 and b[-1] == n and np.all(np.diff(b) > 0) and np.diff(b).max() <= 448
    return b


def capped(b):
    """what the 448-row cap makes of a list of bounds: pieces of 224 rows off the front of a chunk as long as it is above 448"""
    out = [0]
    for x in b[1:]:
        while x - out[-1] > 448:
            out.append(out[-1] + 224)
        if x > out[-1]:
            out.append(x)
    return np.array(out)


def test_chunk_bounds_in_their_three_regimes_and_under_the_cap(program, tmp_path):
    n, target = 1000, 130
    # ranks of ~85 rows: whole ranks, a chunk closed in front of the rank that would take it past the target
    rk = np.array([0, 85, 170, 250, 340, 425, 500, 590, 670, 760, 845, 930, 1000])
    want, start = [0], 0
    for r in range(1, len(rk)):
        if rk[r] - start > target and rk[r - 1] > start:
            want.append(rk[r - 1])
            start = rk[r - 1]
    assert np.array_equal(bounds(program, tmp_path, n, rk, target), want + [n])
    assert np.array_equal(want, [0, 85, 170, 250, 340, 425, 500, 590, 670, 760, 845, 930])      # here: one rank per chunk
    assert np.array_equal(bounds(program, tmp_path, n, rk, 180), [0, 170, 340, 500, 670, 845, 1000])  # two ranks fit a larger target
    # ranks of 300 rows (<= 4 * target): equal parts of at most `target` rows that end on the rank boundaries
    rk = np.array([0, 300, 600, 900, 1000])
    assert np.array_equal(bounds(program, tmp_path, n, rk, target), [0, 100, 200, 300, 400, 500, 600, 700, 800, 900, 1000])
    rk = np.array([0, 301, 600, 600, 1000])                                     # an empty rank, and parts that do not divide
    assert np.array_equal(bounds(program, tmp_path, n, rk, target), [0, 100, 200, 301, 400, 500, 600, 700, 800, 900, 1000])
    # one rank, ranks above 4 * target, or by_rank_allowed = false: the fixed 128
    fixed = np.array(list(range(0, n, 128)) + [n])
    assert np.array_equal(bounds(program, tmp_path, n, [0, n], target), fixed)
    assert np.array_equal(bounds(program, tmp_path, n, [0, 521, n], 124), fixed)                 # 500 rows per rank > 4 * 124 ...
    assert np.array_equal(bounds(program, tmp_path, n, [0, 521, n], 125),                        # ... but = 4 * 125: 521 rows in 5 parts, 479 in 4
                          [0] + [521 * q // 5 for q in range(1, 6)] + [521 + 479 * q // 4 for q in range(1, 5)])
    assert np.array_equal(bounds(program, tmp_path, n, [0, 600, n], 120), fixed)                 # 500 rows per rank > 4 * 120
    assert np.array_equal(bounds(program, tmp_path, n, np.arange(0, 1001, 100), target, allowed=False), fixed)
    assert np.array_equal(bounds(program, tmp_path, 128, [0, 128], target), [0, 128])
    # by rank with an empty rank in the table
    rk = np.array([0, 100, 100, 200, 300, 300, 400, 500, 600, 700, 800, 900, 1000])
    assert np.array_equal(bounds(program, tmp_path, n, rk, target), np.arange(0, 1001, 100))
    # the cap: a by-rank chunk of 950 rows (one oversized rank among small ones) is cut into pieces of 224
    rk = np.array([0, 10, 960, 970, 980, 985, 990, 992, 994, 996, 998, 1000])
    b = bounds(program, tmp_path, n, rk, 100)
    assert np.array_equal(b, capped([0, 10, 960, 1000])) and np.array_equal(b, [0, 10, 234, 458, 682, 960, 1000])
    assert np.array_equal(bounds(program, tmp_path, n, [0, 449, 898, n], 448), [0, 224, 449, 673, 898, 1000])   # split ranks of 449 rows


# ---------------------------------------------------------------- chunk table
def check_chunks(program, tmp_path, g, bd, n_own, largest_first):
    n = g.shape[0]
    bd = np.asarray(bd)
    head, out = run(program, tmp_path, "chunks", [n, n_own, int(largest_first), len(bd)], g.indptr, g.indices, bd)
    assert head[0] == "ok"
    n_chunks, max_ucols, max_rows, grid, grid_if, n_chunks_if = (int(x) for x in head[1:7])
    cptr, ucols, lidx, desc, order, desc_if = out
    assert n_chunks == len(bd) - 1 and max_rows == np.diff(bd).max()
    nnz_of = g.indptr[bd[1:]] - g.indptr[bd[:-1]]
    ghost = np.zeros(n_chunks, dtype=bool)
    for c in range(n_chunks):
        cols = g.indices[g.indptr[bd[c]]:g.indptr[bd[c + 1]]]
        assert np.array_equal(ucols[cptr[c]:cptr[c + 1]], np.unique(cols))
        assert np.array_equal(ucols[cptr[c] + lidx[g.indptr[bd[c]]:g.indptr[bd[c + 1]]]], cols)
        ghost[c] = len(cols) > 0 and cols.max() >= n_own
    assert max_ucols == np.diff(cptr).max() and len(lidx) == g.nnz
    assert n_chunks_if == ghost.sum() and float(head[7]) == (nnz_of[ghost].sum() / g.nnz if g.nnz else 0.0)
    seen = []
    for table, n_wg, chunks, chunk_of in ((desc, grid, np.flatnonzero(~ghost), order), (desc_if, grid_if, np.flatnonzero(ghost), None)):
        if len(chunks) == 0 and chunk_of is None:
            assert n_wg == 0 and len(table) == 0
            continue
        # XCD k takes the chunks [cut[k], cut[k+1]) of the list: the running count of non-zeros passes k / 8 of the total
        run_nnz, total = np.cumsum(nnz_of[chunks]), nnz_of[chunks].sum()
        cut = [0] + [int(np.sum(run_nnz * 8 <= total * k)) for k in range(1, 8)] + [len(chunks)]
        assert n_wg == 8 * max(np.diff(cut)) and len(table) == 4 * n_wg
        want = np.full(n_wg, -1)
        for k in range(8):
            mine = chunks[cut[k]:cut[k + 1]]
            if largest_first:
                mine = mine[np.argsort(-nnz_of[mine], kind="stable")]
            want[8 * np.arange(len(mine)) + k] = mine
        rec = table.reshape(n_wg, 4)
        live = want >= 0
        c = want[live]
        assert np.array_equal(rec[live], np.stack([cptr[c], cptr[c + 1] - cptr[c], bd[c], bd[c + 1]], axis=1))
        assert not rec[~live].any()                                             # padding records are all zero
        if chunk_of is not None:
            assert np.array_equal(chunk_of, want)
        seen += list(c)
    assert sorted(seen) == list(range(n_chunks))                                # every chunk once across the two tables
    return ghost


@pytest.mark.parametrize("mesh", MESHES)
def test_chunk_table_stages_the_unique_columns_and_deals_the_chunks_to_the_xcds(program, tmp_path, mesh):
    g = graphs(mesh).A
    n = g.shape[0]
    step = 130 if n > 1000 else 7
    bd = np.array(list(range(0, n, step)) + [n])
    for largest_first in (True, False):
        assert not check_chunks(program, tmp_path, g, bd, n, largest_first).any()
    # a distributed handle's view: the rows of the first 70 % of the nodes, all columns; the chunks that reach a column >= n_own wait
    n_own = (7 * n) // 10
    own = pattern(g[:n_own])
    bd = np.array(list(range(0, n_own, step)) + [n_own])
    for largest_first in (True, False):
        ghost = check_chunks(program, tmp_path, own, bd, n_own, largest_first)
        assert ghost.any() and not ghost.all()


def test_chunk_table_reports_a_chunk_of_more_than_65535_columns(program, tmp_path):
    for n_cols, word in ((65535, "ok"), (65536, "toomany")):
        g = sp.csr_matrix((np.ones(n_cols + 1), (np.array([0] * n_cols + [1]), np.array(list(range(n_cols)) + [0]))), shape=(2, n_cols))
        head, out = run(program, tmp_path, "chunks", [2, n_cols, 1, 2], g.indptr, g.indices, [0, 2])
        assert head[0] == word
        if word == "ok":
            assert np.array_equal(out[2], list(range(n_cols)) + [0]) and int(head[2]) == 65535
        else:
            assert out == []


# ---------------------------------------------------------------- gather map
def check_gather(program, tmp_path, g, n_rows, cr, cc, stride, swapped):
    n_cells, per_r, per_c = cr.shape[0], cr.shape[1], cc.shape[1]
    g = pattern(g[:n_rows])
    head, out = run(program, tmp_path, "gather", [n_rows, n_cells, per_r, per_c, stride, int(swapped)], g.indptr, g.indices, cr, cc)
    assert head == ["ok"]
    ptr, src = out
    want = {}
    for c in range(n_cells):
        for a in range(per_r):
            if cr[c, a] >= n_rows:
                continue                                                        # ghost row: nothing
            for b in range(per_c):
                plane = b * per_r + a if swapped else a * per_c + b
                want.setdefault((cr[c, a], cc[c, b]), []).append(plane * stride * n_cells + c)
    rows = np.repeat(np.arange(n_rows), np.diff(g.indptr))
    assert len(ptr) == g.nnz + 1 and ptr[0] == 0 and ptr[-1] == len(src) == sum(len(v) for v in want.values())
    assert len(want) == g.nnz
    for e in range(g.nnz):
        assert np.array_equal(src[ptr[e]:ptr[e + 1]], want[(rows[e], g.indices[e])])
        assert np.all(np.diff(src[ptr[e]:ptr[e + 1]] % n_cells) > 0)            # ascending cell order, a cell at most once


@pytest.mark.parametrize("mesh", MESHES[:2])
def test_gather_lists_hold_every_contribution_in_cell_order(program, tmp_path, mesh):
    m = graphs(mesh)
    check_gather(program, tmp_path, m.A, m.N2, m.c2, m.c2, 1, False)
    check_gather(program, tmp_path, m.G, m.N2, m.c2, m.c1, m.dim, False)        # planes (a * np1 + v) * dim
    check_gather(program, tmp_path, m.B, m.NP, m.c1, m.c2, m.dim, True)         # the same planes, indexed (v, a)
    check_gather(program, tmp_path, m.A, (2 * m.N2) // 3, m.c2, m.c2, 1, False)  # the last third of the nodes are ghosts: their rows get nothing
    check_gather(program, tmp_path, m.B, m.NP - 3, m.c1, m.c2, m.dim, True)


def test_gather_reports_a_pair_outside_the_graph_and_an_offset_beyond_int32(program, tmp_path):
    m = graphs(MESHES[0])
    g = m.A.tolil()
    g[m.c2[4, 0], m.c2[4, 5]] = 0
    g = pattern(g.tocsr())
    g.eliminate_zeros()
    head, out = run(program, tmp_path, "gather", [m.N2, m.n_cells, 6, 6, 1, 0], g.indptr, g.indices, m.c2, m.c2)
    assert head == ["missing"] and out == []
    head, out = run(program, tmp_path, "gather", [m.N2, m.n_cells, 6, 6, 2 ** 22, 0], m.A.indptr, m.A.indices, m.c2, m.c2)
    assert head == ["overflow"] and out == []                                   # plane 35 * 2^22 * 18 cells > 2^31


# ---------------------------------------------------------------- Schur pattern
def check_schur(program, tmp_path, B, n_rows):
    head, out = run(program, tmp_path, "schur", [B.shape[0], B.shape[1], n_rows, B.shape[0]], B.indptr, B.indices)
    assert head == ["ok"]
    absB = sp.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)
    want = pattern((absB @ absB.T)[:n_rows])
    assert np.array_equal(out[0], want.indptr) and np.array_equal(out[1], want.indices)
    assert all(np.all(np.diff(out[1][out[0][i]:out[0][i + 1]]) > 0) for i in range(n_rows))     # columns sorted


@pytest.mark.parametrize("mesh", MESHES)
def test_schur_pattern_is_the_pattern_of_b_bt_on_the_owned_rows(program, tmp_path, mesh):
    B = graphs(mesh).B
    check_schur(program, tmp_path, B, B.shape[0])
    check_schur(program, tmp_path, B, (2 * B.shape[0]) // 3)                    # B also holds ghost rows behind the owned ones
