"""CPU suite: host/adjacency.hpp (the face-neighbour table behind the tracer particles' walk) through a stand-alone program,
tests/adjacency_check.cpp, built here with AddressSanitizer and UBSan, against the Python adjacency of tests/tracer_reference.py."""
import os
import subprocess

import numpy as np
import pytest

import tracer_reference as TR
from conftest import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adjacency") / "adjacency_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "adjacency_check.cpp")], check=True)
    return exe


def run(program, cells, tmp_path):
    cells = np.asarray(cells)
    path = tmp_path / "cells.txt"
    with open(path, "w") as f:
        f.write("%d %d\n" % cells.shape)
        np.savetxt(f, cells, fmt="%d")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]      # a sanitizer report ends the program with a status of its own
    head, _, rest = r.stdout.partition("\n")
    if head != "ok":
        return head, None
    return head, np.array(rest.split(), dtype=np.int64).reshape(cells.shape[1], cells.shape[0])


@pytest.mark.parametrize("kind,dim,n_cells", [("box", 2, 18), ("box", 3, 108), ("cube", 3, 6)])
def test_table_equals_the_python_adjacency(program, tmp_path, kind, dim, n_cells):
    p = Problem(kind, dim, 1) if kind == "cube" else Problem(kind, dim)
    assert p.dofs.n_cells == n_cells
    head, nbr = run(program, p.mesh.cells, tmp_path)
    assert head == "ok"
    ref = TR.adjacency(p.mesh.cells)
    assert np.array_equal(nbr, ref)
    assert (nbr == -1).sum() == len(p.mesh.bfaces) and (nbr >= 0).any()
    # a renumbering of the vertices changes no neighbour (the library hands over P1 node ids, not mesh vertex ids)
    perm = np.random.default_rng(5).permutation(int(p.mesh.cells.max()) + 1)
    assert np.array_equal(run(program, perm[p.mesh.cells], tmp_path)[1], ref)


def test_a_face_with_three_cells_is_refused(program, tmp_path):
    """three tetrahedra around the face {0, 1, 2}, behind a regular pair; three triangles around the edge {0, 1}"""
    tets = [[7, 8, 9, 10], [7, 8, 9, 11], [0, 1, 2, 3], [0, 1, 2, 4], [2, 0, 1, 5]]
    assert run(program, tets, tmp_path)[0] == "refused 2"
    assert run(program, tets[:4], tmp_path)[0] == "ok"
    with pytest.raises(ValueError):
        TR.adjacency(tets)
    tris = [[0, 1, 2], [1, 0, 3], [0, 1, 4]]
    assert run(program, tris, tmp_path)[0] == "refused 0"
    assert run(program, [[0, 1, 1]], tmp_path)[0] == "refused 0"          # a repeated vertex: one face twice in one cell
    assert run(program, [[0, -1, 2]], tmp_path)[0] == "bad"
    head, nbr = run(program, np.zeros((0, 4), dtype=int), tmp_path)
    assert head == "ok" and nbr.size == 0
