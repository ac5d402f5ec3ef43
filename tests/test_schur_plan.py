"""CPU suite: the planner of the Schur product (host/schur_plan.hpp) through a stand-alone program, tests/schur_plan_check.cpp, built
here with AddressSanitizer and UBSan.  For every entry (i, j) of S the plan must list exactly the columns rows i and j of B share, in
row j's ascending order, as (position in row i, offset in row j); a replay of the plan must give, bit for bit, what a replay of
k_schur's merge gives (one term function for both, weights with exact zeros among them).  Patterns: random sorted ones (S with entries
whose rows share nothing, a row of more than 64 entries: a second group) and the graphs of the front-end's 3D level-1 cylinder."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import nodal_reference as NR
from conftest import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TERM = 0xFFFFFFFF


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schur_plan") / "schur_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "schur_plan_check.cpp")], check=True)
    return exe


def run(program, tmp_path, command, head, S, B):
    path = tmp_path / "input.txt"
    with open(path, "w") as f:
        for a in (head, S.indptr, S.indices, B.indptr, B.indices):
            f.write(" ".join(str(int(x)) for x in np.asarray(a).ravel()) + "\n")
    r = subprocess.run([program, command, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]      # a sanitizer report ends the program with a status of its own
    lines = r.stdout.split("\n")
    return lines[0].split(), [np.array(s.split(), dtype=np.int64) for s in lines[1:-1]]


def pattern(m):
    m = sp.csr_matrix(m)
    m.sum_duplicates()
    m.sort_indices()
    return m


def check_plan(program, tmp_path, S, B):
    """the plan of (S, B) against the set intersections; returns (matches, groups, entries without a term)"""
    head, out = run(program, tmp_path, "plan", [S.shape[0], S.shape[1], B.shape[0], B.shape[1], 0], S, B)
    assert head[0] == "ok", head
    max_row, entries, matches, slots = (int(x) for x in head[1:])
    row_grp, grp_off, words = out
    assert max_row == np.diff(B.indptr).max() and entries == S.nnz and slots == len(words) == grp_off[-1]
    per_row = np.diff(S.indptr)
    assert row_grp[0] == 0 and np.array_equal(np.diff(row_grp), (per_row + 63) // 64) and len(grp_off) == row_grp[-1] + 1
    assert grp_off[0] == 0 and np.all(np.diff(grp_off) >= 0) and np.all(grp_off % 64 == 0)
    total, empty = 0, 0
    for i in range(S.shape[0]):
        ri = B.indices[B.indptr[i]:B.indptr[i + 1]]
        longest = {}
        for e in range(S.indptr[i], S.indptr[i + 1]):
            j = S.indices[e]
            rj = B.indices[B.indptr[j]:B.indptr[j + 1]]
            local = e - S.indptr[i]
            g, lane = row_grp[i] + local // 64, local % 64
            lane_words = words[grp_off[g] + lane:grp_off[g + 1]:64]
            live = lane_words[lane_words != NO_TERM]
            assert np.all(lane_words[len(live):] == NO_TERM)                        # the terms first, then nothing
            shared, qi, pj = np.intersect1d(ri, rj, assume_unique=True, return_indices=True)     # ascending: row j's own order
            assert np.array_equal(live >> 16, qi) and np.array_equal(live & 0xFFFF, pj), (i, j)
            total += len(shared)
            empty += len(shared) == 0
            longest[g] = max(longest.get(g, 0), len(shared))
        for g in range(row_grp[i], row_grp[i + 1]):
            assert grp_off[g + 1] - grp_off[g] == 64 * longest[g]                   # as many steps as the longest lane
            tail = per_row[i] - 64 * (g - row_grp[i])
            if tail < 64:                                                          # lanes behind the row's last entry: nothing
                slab = words[grp_off[g]:grp_off[g + 1]].reshape(-1, 64)
                assert np.all(slab[:, tail:] == NO_TERM)
    assert total == matches
    return matches, int(row_grp[-1]), empty


def check_replay(program, tmp_path, S, B, dim, seed):
    head, out = run(program, tmp_path, "replay", [S.shape[0], S.shape[1], B.shape[0], B.shape[1], dim, seed], S, B)
    assert head[0] == "same" and int(head[1]) == S.nnz, head
    return int(head[2])


def random_pattern(rng, n_rows, n_cols, lo, hi):
    rows = [np.sort(rng.choice(n_cols, size=rng.integers(lo, hi + 1), replace=False)) for _ in range(n_rows)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return sp.csr_matrix((np.ones(ptr[-1]), np.concatenate(rows) if ptr[-1] else np.zeros(0, int), ptr), shape=(n_rows, n_cols))


def product_pattern(B, n_rows):
    a = sp.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)
    return pattern((a @ a.T)[:n_rows])


@pytest.mark.parametrize("seed", [1, 2])
def test_random_patterns_with_empty_intersections_and_a_second_group(program, tmp_path, seed):
    rng = np.random.default_rng(seed)
    B = random_pattern(rng, 150, 400, 0, 30)                       # rows of 0 .. 30 columns, empty ones among them
    S = pattern(sp.csr_matrix(np.ones((150, 150))))                # every pair: most rows share nothing; 150 entries per row = 3 groups
    matches, groups, empty = check_plan(program, tmp_path, S, B)
    assert groups == 150 * 3 and empty > 0 and matches > 0
    for dim in (2, 3):
        assert check_replay(program, tmp_path, S, B, dim, seed) >= empty       # no term at all: exactly 0.0
    S = product_pattern(B, 100)                                    # the structural product on the first 100 rows (B holds "ghost" rows behind them)
    matches, groups, empty = check_plan(program, tmp_path, S, B)
    assert empty == 0 and np.diff(S.indptr).max() > 64
    check_replay(program, tmp_path, S, B, 3, seed)


def test_the_graphs_of_the_3d_level_1_cylinder(program, tmp_path):
    p = Problem("cylinder", 3, 1)
    d, dim = p.dofs, 3
    n_cells = d.n_cells
    c2 = NR.cell_nodes(d)
    c1 = np.asarray(d.cell_dofs)[:, [(dim + 1) * v + dim for v in range(dim + 1)]] - d.n_u
    inc = lambda c, n: sp.csr_matrix((np.ones(c.size), (np.repeat(np.arange(n_cells), c.shape[1]), c.ravel())), shape=(n_cells, n))
    B = pattern(inc(c1, d.n_p).T @ inc(c2, d.n_u // dim))
    S = product_pattern(B, d.n_p)
    assert S.shape == (745, 745) and np.diff(S.indptr).max() == 76 and np.diff(B.indptr).max() > 64
    matches, groups, empty = check_plan(program, tmp_path, S, B)
    assert empty == 0 and groups == 745 + int(np.sum(np.diff(S.indptr) > 64))
    zeros = check_replay(program, tmp_path, S, B, dim, 7)
    print("3D level-1 cylinder: %d entries, %d terms (%.1f per entry), %d groups, %d exact zeros in the replay" % (S.nnz, matches, matches / S.nnz, groups, zeros))


def test_a_plan_beyond_the_word_limit_is_given_up(program, tmp_path):
    rng = np.random.default_rng(5)
    B = random_pattern(rng, 40, 90, 3, 20)
    S = product_pattern(B, 40)
    head, out = run(program, tmp_path, "plan", [40, 40, 40, 90, 0], S, B)
    slots = int(head[4])
    for limit, word in ((slots, "ok"), (slots - 1, "refused")):
        head, out = run(program, tmp_path, "plan", [40, 40, 40, 90, limit], S, B)
        assert head[0] == word and (word == "ok") == (len(out) == 3)


def test_rows_of_65535_entries_are_refused(program, tmp_path):
    for n_cols, word in ((65534, "ok"), (65535, "refused")):
        B = sp.csr_matrix((np.ones(n_cols + 1), (np.array([0] * n_cols + [1]), np.array(list(range(n_cols)) + [n_cols - 1]))), shape=(2, n_cols))
        S = pattern(sp.csr_matrix(np.ones((2, 2))))
        head, out = run(program, tmp_path, "plan", [2, 2, 2, n_cols, 0], S, B)
        assert head[0] == word and int(head[1]) == n_cols
        if word == "ok":
            row_grp, grp_off, words = out
            assert np.array_equal(row_grp, [0, 1, 2]) and np.array_equal(grp_off, [0, 64 * n_cols, 64 * n_cols + 64])
            slab = words[:64 * n_cols].reshape(-1, 64)
            assert np.array_equal(slab[:, 0], (np.arange(n_cols) << 16) | np.arange(n_cols))          # (0, 0): the whole row, the largest positions
            assert slab[0, 1] == ((n_cols - 1) << 16 | 0) and np.all(slab[1:, 1] == NO_TERM) and np.all(slab[:, 2:] == NO_TERM)
            assert words[64 * n_cols] == (0 << 16 | n_cols - 1) and words[64 * n_cols + 1] == 0       # (1, 0) and (1, 1)
        else:
            assert out == []
