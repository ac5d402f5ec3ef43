"""CPU suite: host/nodal_patch.hpp (the node -> (cell, local node) table behind nsx_compute_nodal_fields) through a stand-alone program,
tests/nodal_patch_check.cpp, built here with AddressSanitizer and UBSan, against lists made from the connectivity in Python.  The table is
replayed the way the kernel walks it: tile by tile, step by step, lane by lane."""
import os
import subprocess

import numpy as np
import pytest

import nodal_reference as NR
from conftest import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nodal_patch") / "nodal_patch_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "nodal_patch_check.cpp")], check=True)
    return exe


def run(program, cells, n_nodes, tmp_path):
    cells = np.asarray(cells)
    path = tmp_path / "cells.txt"
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (cells.shape[0], cells.shape[1], n_nodes))
        np.savetxt(f, cells, fmt="%d")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]      # a sanitizer report ends the program with a status of its own
    lines = r.stdout.split("\n")
    if not lines[0].startswith("ok"):
        return lines[0], None
    n_tiles, max_size, n_pairs = (int(x) for x in lines[0].split()[1:])
    size, order, tile_ptr, ent = (np.array(s.split(), dtype=np.int64) for s in lines[1:5])
    return "ok", dict(n_tiles=n_tiles, max_size=max_size, n_pairs=n_pairs, size=size, order=order, tile_ptr=tile_ptr, ent=ent.reshape(-1, 64))


def replay(t):
    """{node: [(cell, local node), ...]} in the order in which lane `slot % 64` of tile `slot // 64` meets the entries"""
    lists = {}
    for tile in range(t["n_tiles"]):
        for lane in range(64):
            node = t["order"][tile * 64 + lane]
            col = t["ent"][t["tile_ptr"][tile]:t["tile_ptr"][tile + 1], lane]
            live = col[col >= 0]
            assert np.array_equal(col[:len(live)], live)                # padding only behind the list
            if node < 0:
                assert len(live) == 0
                continue
            assert node not in lists
            lists[int(node)] = [(int(e) >> 4, int(e) & 15) for e in live]
    return lists


def expected(cells, n_nodes):
    lists = {n: [] for n in range(n_nodes)}
    for c, row in enumerate(np.asarray(cells)):
        for a, n in enumerate(row):
            if n < n_nodes:
                lists[int(n)].append((c, a))
    return lists


@pytest.mark.parametrize("kind,dim,n_cells", [("box", 2, 18), ("box", 3, 108), ("cube", 3, 6), ("cylinder", 3, 2832)])
def test_table_replays_to_the_lists_of_the_connectivity(program, tmp_path, kind, dim, n_cells):
    p = Problem(kind, dim, 1) if kind != "box" else Problem(kind, dim)
    assert p.dofs.n_cells == n_cells
    cn = NR.cell_nodes(p.dofs)
    n_nodes = p.dofs.n_u // dim
    head, t = run(program, cn, n_nodes, tmp_path)
    assert head == "ok"
    want = expected(cn, n_nodes)
    assert replay(t) == want                                            # every node once, its cells ascending
    sizes = np.array([len(want[n]) for n in range(n_nodes)])
    assert np.array_equal(t["size"], sizes) and t["max_size"] == sizes.max() and t["n_pairs"] == cn.size
    assert t["n_tiles"] == -(-n_nodes // 64)
    live = t["order"][t["order"] >= 0]
    assert np.array_equal(t["order"][:n_nodes], live) and np.all(np.diff(sizes[live]) <= 0)     # descending patch size over the slots
    assert np.array_equal(np.diff(t["tile_ptr"]), sizes[t["order"][::64]])                       # a tile runs as long as its longest list
    # the padding the size order leaves: less than one step per tile beyond the pairs
    assert t["ent"].size - t["n_pairs"] <= 64 * (t["n_tiles"] + t["max_size"])


def test_ghost_nodes_get_no_patch_and_bad_input_is_refused(program, tmp_path):
    cells = [[0, 1, 2, 5, 6, 7], [2, 1, 3, 6, 8, 9], [4, 3, 1, 9, 8, 10]]
    head, t = run(program, cells, 5, tmp_path)                          # nodes 5.. are another rank's
    assert head == "ok" and replay(t) == expected(cells, 5) and t["n_pairs"] == 9 and t["n_tiles"] == 1
    assert replay(t)[1] == [(0, 1), (1, 1), (2, 2)]
    head, t = run(program, cells, 13, tmp_path)                         # nodes 11 and 12 are in no cell
    assert head == "ok" and replay(t)[12] == [] and t["size"][11] == 0
    assert run(program, [[0, -1, 2]], 3, tmp_path)[0] == "bad"
    assert run(program, np.zeros((1, 17), dtype=int), 1, tmp_path)[0] == "bad"                   # more local nodes than an entry can name
    head, t = run(program, np.zeros((0, 6), dtype=int), 0, tmp_path)
    assert head == "ok" and t["n_tiles"] == 0 and t["ent"].size == 0
