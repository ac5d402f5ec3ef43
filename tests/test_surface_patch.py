"""CPU suite: host/surface_patch.hpp (the surface-node table, the node -> (face, face node) patch lists and the block tables of the fold
behind nsx_set_surface) through a stand-alone program, tests/surface_patch_check.cpp, built here with AddressSanitizer and UBSan and run as a
child process, on the face lists of the box and cylinder meshes.  The table is replayed the way the kernel walks it."""
import os
import subprocess

import numpy as np
import pytest

import surface_reference as SR
from conftest import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("surface_patch") / "surface_patch_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "surface_patch_check.cpp")], check=True)
    return exe


def run(program, node_of, groups, n_groups, tmp_path):
    node_of = np.asarray(node_of)
    node_of = node_of.reshape(len(groups), node_of.shape[-1])
    path = tmp_path / "faces.txt"
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (node_of.shape[0], node_of.shape[1], n_groups))
        np.savetxt(f, np.column_stack([np.asarray(groups).reshape(-1, 1), node_of]) if len(groups) else np.zeros((0, 1)), fmt="%d")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]      # a sanitizer report ends the program with a status of its own
    lines = r.stdout.split("\n")
    if not lines[0].startswith("ok"):
        return lines[0], None
    n_nodes, n_tiles, max_size = (int(x) for x in lines[0].split()[1:])
    keys = ("order", "group_ptr", "node_id", "node_group", "face_nodes", "size", "slot_of", "tile_ptr", "ent")
    t = {k: np.array(s.split(), dtype=np.int64) for k, s in zip(keys, lines[1:10])}
    levels = int(lines[10])
    t["fold"] = [np.array(s.split(), dtype=np.int64).reshape(-1, 3) for s in lines[11:11 + levels]]
    t.update(n_nodes=n_nodes, n_tiles=n_tiles, max_size=max_size, ent=t["ent"].reshape(-1, 64))
    t["face_nodes"] = t["face_nodes"].reshape(node_of.shape)
    return "ok", t


def replay(t):
    """{surface node: [(sorted face position, face node), ...]} in the order in which its lane meets the entries"""
    node_at = np.full(t["n_tiles"] * 64, -1, dtype=np.int64)
    node_at[t["slot_of"]] = np.arange(t["n_nodes"])
    assert len(np.unique(t["slot_of"])) == t["n_nodes"]
    lists = {}
    for tile in range(t["n_tiles"]):
        for lane in range(64):
            s = node_at[tile * 64 + lane]
            col = t["ent"][t["tile_ptr"][tile]:t["tile_ptr"][tile + 1], lane]
            live = col[col >= 0]
            assert np.array_equal(col[:len(live)], live)                # padding only behind the list
            if s < 0:
                assert len(live) == 0
                continue
            lists[int(s)] = [(int(e) >> 3, int(e) & 7) for e in live]
    return lists, node_at


def check(t, node_of, groups, n_groups):
    node_of, groups = np.asarray(node_of), np.asarray(groups)
    nf, npf = node_of.shape
    # the faces stable-sorted by group
    assert np.array_equal(t["order"], np.argsort(groups, kind="stable"))
    assert np.array_equal(t["group_ptr"], np.concatenate([[0], np.cumsum(np.bincount(groups, minlength=n_groups))]))
    # the surface nodes: distinct (group, node) pairs, ascending group then node; a seam node once per group
    pairs = sorted({(int(g), int(n)) for g, row in zip(groups, node_of) for n in row})
    assert t["n_nodes"] == len(pairs)
    assert list(zip(t["node_group"].tolist(), t["node_id"].tolist())) == pairs
    for f in range(nf):
        for j in range(npf):
            s = t["face_nodes"][f, j]
            assert (t["node_group"][s], t["node_id"][s]) == (groups[f], node_of[f, j])
    # every (face, face node) exactly once, in the list of its surface node, faces ascending
    lists, node_at = replay(t)
    seen = set()
    for s, entries in lists.items():
        assert len(entries) == t["size"][s]
        pos = [p for p, _ in entries]
        assert pos == sorted(pos) and len(set(pos)) == len(pos)         # ascending sorted position = ascending caller position in a group
        for p, j in entries:
            f = t["order"][p]
            assert t["face_nodes"][f, j] == s and (f, j) not in seen
            seen.add((int(f), j))
        caller = [int(t["order"][p]) for p, _ in entries]
        assert caller == sorted(caller)
    assert len(seen) == nf * npf
    live = node_at[node_at >= 0]
    assert np.array_equal(node_at[:t["n_nodes"]], live) and np.all(np.diff(t["size"][live]) <= 0)   # descending patch size over the slots
    assert t["n_tiles"] == -(-t["n_nodes"] // 64) and t["max_size"] == (t["size"].max() if t["n_nodes"] else 0)
    if t["n_tiles"]:
        assert np.array_equal(np.diff(t["tile_ptr"]), t["size"][node_at[::64]])
    # the fold: per level every group's entries in blocks of 64, until one entry per group is left
    ptr = t["group_ptr"]
    for lvl in t["fold"]:
        nxt, k = [0], 0
        for g in range(n_groups):
            a, b = ptr[g], ptr[g + 1]
            nb = max(1, -(-(b - a) // 64))
            for i in range(nb):
                assert lvl[k].tolist() == [a + 64 * i, min(b, a + 64 * (i + 1)), g]
                k += 1
            nxt.append(nxt[-1] + nb)
        assert k == len(lvl)
        ptr = np.array(nxt)
    assert np.array_equal(ptr, np.arange(n_groups + 1))
    assert len(t["fold"]) == max(SR.fold_depth(int(c)) for c in np.diff(t["group_ptr"])) // 6


@pytest.mark.parametrize("kind,dim,level", [("box", 2, 1), ("box", 3, 1), ("cylinder", 2, 1), ("cylinder", 3, 1)])
def test_tables_of_the_mesh_boundaries(program, tmp_path, kind, dim, level):
    from navierstokes_project_nm4pde_amd.problem import boundary_faces
    p = Problem(kind, dim) if kind == "box" else Problem(kind, dim, level)
    cells, lfs, groups = boundary_faces(p.mesh)
    lay = SR.layout(p.dofs, cells, lfs, groups)
    n_groups = int(groups.max()) + 1
    node_of = lay["nodes"][lay["face_nodes"]]
    head, t = run(program, node_of, groups, n_groups, tmp_path)
    assert head == "ok"
    check(t, node_of, groups, n_groups)
    assert np.array_equal(t["face_nodes"], lay["face_nodes"]) and np.array_equal(t["node_id"], lay["nodes"])   # the helper's numbering
    assert t["n_nodes"] > len(np.unique(node_of))                       # the seam nodes are doubled
    if kind == "cylinder" and dim == 3:
        assert len(cells) == 968 and len(t["fold"]) == 2 and (t["size"].min(), t["size"].max()) == (1, 7)   # corner nodes to vertex fans
        assert (np.bincount(cells) == 2).sum() == 70


def test_small_sets_and_bad_input(program, tmp_path):
    node_of = [[0, 1, 5], [1, 2, 6], [2, 3, 7], [3, 0, 8]]
    head, t = run(program, node_of, [1, 0, 1, 0], 3, tmp_path)          # group 2 has no face
    assert head == "ok"
    check(t, node_of, [1, 0, 1, 0], 3)
    assert t["order"].tolist() == [1, 3, 0, 2] and t["group_ptr"].tolist() == [0, 2, 4, 4] and t["n_nodes"] == 12
    assert t["fold"][0].tolist() == [[0, 2, 0], [2, 4, 1], [4, 4, 2]] and len(t["fold"]) == 1
    head, t = run(program, np.arange(130 * 3).reshape(130, 3), [0] * 130, 1, tmp_path)   # three blocks, two levels
    assert head == "ok" and [len(l) for l in t["fold"]] == [3, 1] and t["fold"][0][2].tolist() == [128, 130, 0]
    assert run(program, node_of, [0, 0, 0, 3], 3, tmp_path)[0] == "bad"                   # a group out of range
    assert run(program, node_of, [0, 0, 0, 0], 0, tmp_path)[0] == "bad" and run(program, node_of, [0, 0, 0, 0], 65, tmp_path)[0] == "bad"
    assert run(program, [[0, -1, 2]], [0], 1, tmp_path)[0] == "bad"
    assert run(program, np.zeros((1, 7), dtype=int), [0], 1, tmp_path)[0] == "bad"        # more face nodes than an entry can name
    head, t = run(program, np.zeros((0, 3), dtype=int), [], 2, tmp_path)
    assert head == "ok" and t["n_nodes"] == 0 and t["n_tiles"] == 0 and t["ent"].size == 0
