"""CPU suite: host/iso_tables.hpp (the case tables behind nsx_extract_isosurface) through a stand-alone program, tests/iso_tables_check.cpp,
built here with AddressSanitizer and UBSan.  Every case is checked by its properties -- the crossings join an inside to an outside vertex, the
count, the orientation on the unit simplex -- and against the table tests/iso_reference.py builds from the header's rule."""
import os
import subprocess

import numpy as np
import pytest

import iso_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("iso_tables") / "iso_tables_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "iso_tables_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]          # a sanitizer report ends the program with a status of its own
    out = {"sub2": [], "sub3": [], "tri": {}, "tet": {}}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] in ("sub2", "sub3"):
            out[w[0]].append(tuple(int(x) for x in w[1:]))
        elif w[0] in ("tri", "tet"):
            per = 2 if w[0] == "tri" else 3
            m, n = int(w[1]), int(w[2])
            edges = [tuple(int(x) for x in e.split("-")) for e in w[3:]]
            assert len(edges) == per * n
            out[w[0]][m] = [edges[per * k:per * (k + 1)] for k in range(n)]
        elif w[0] == "max":
            out["max"] = (int(w[1]), int(w[2]))
    return out


def test_subdivision_is_the_headers(tables):
    assert tables["sub2"] == IR.SUB[2] and tables["sub3"] == IR.SUB[3]
    assert tables["max"] == (4, 16)
    # in reference coordinates every sub-simplex has the orientation of the cell and an equal share of it
    for dim, subs in ((2, tables["sub2"]), (3, tables["sub3"])):
        P = IR.UNIT[dim]
        nodes = np.concatenate([P, np.array([(P[i] + P[j]) / 2 for i, j in IR.LINES[dim]])])
        for loc in subs:
            Q = nodes[list(loc)]
            assert np.isclose(np.linalg.det(Q[1:] - Q[0]), 1.0 / len(subs))
    # a face of the tetrahedron is cut into the canonical 4 triangles: the faces of the sub-tetrahedra that lie in it
    for face in ((0, 1, 2), (0, 1, 3), (1, 2, 3), (0, 2, 3)):
        on = set(face) | {4 + e for e, (i, j) in enumerate(IR.LINES[3]) if i in face and j in face}
        pieces = {frozenset(f) for loc in tables["sub3"] for f in ((loc[0], loc[1], loc[2]), (loc[0], loc[1], loc[3]), (loc[0], loc[2], loc[3]), (loc[1], loc[2], loc[3]))
                  if set(f) <= on}
        mids = sorted(on - set(face))
        want = {frozenset(mids)} | {frozenset([v] + [4 + e for e, (i, j) in enumerate(IR.LINES[3]) if v in (i, j) and 4 + e in on]) for v in face}
        assert pieces == want, face


@pytest.mark.parametrize("dim", [2, 3])
def test_every_case(tables, dim):
    table = tables["tri" if dim == 2 else "tet"]
    assert sorted(table) == list(range(1 << (dim + 1)))
    for m, prims in table.items():
        ins = [v for v in range(dim + 1) if m >> v & 1]
        want = 0 if len(ins) in (0, dim + 1) else (2 if (dim == 3 and len(ins) == 2) else 1)
        assert len(prims) == want, m
        for prim in prims:
            assert len(set(prim)) == dim
            for a, b in prim:
                assert (m >> a & 1) and not (m >> b & 1), (m, prim)      # from an inside to an outside vertex
            assert IR.orientation_ok(dim, prim, ins), (m, prim)
        if want == 2:                                                       # the quad i-k i-l j-l j-k split along its first and third corner
            (i, j), (k, l) = ins, [v for v in range(4) if v not in ins]
            quad = [(i, k), (i, l), (j, l), (j, k)]
            assert prims[0][0] == prims[1][0] == quad[0] and quad[2] in prims[0] and quad[2] in prims[1]
            assert set(prims[0]) | set(prims[1]) == set(quad)
        assert prims == IR.TABLE[dim][m], m                                 # and the very order the restatement derives from the rule
