"""CPU suite: host/lattice_box.hpp (the index box behind nsx_set_lattice: which lattice points a cell's rasterisation visits) through a
stand-alone program, tests/lattice_box_check.cpp, built here with AddressSanitizer and UBSan and run directly.  The program draws seeded
random triangles and tetrahedra (slivers, needles, cells far from the origin, cells larger and smaller than the spacing) and random lattices of
at most 40 points per axis, runs the containment test in long double over every lattice point for tol in {0, 1e-12, 1e-6, 0.05, 0.5} and
asserts that no accepted point lies outside the box, that an empty clamp gives an empty box, and that the boxes are not vacuous."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tally(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lattice_box") / "lattice_box_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "lattice_box_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]          # a failed check or a sanitizer report ends it with a status of its own
    out = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "dim":
            out[int(w[1])] = {w[k]: int(w[k + 1]) for k in range(2, len(w), 2)}
        elif w[0] == "failures":
            out["failures"] = int(w[1])
    return out


def test_no_accepted_point_lies_outside_its_box(tally):
    assert tally["failures"] == 0
    for dim in (2, 3):
        t = tally[dim]
        assert t["cases"] >= 3000 and t["accepted"] > 20000, t               # five tolerances per cell and lattice


def test_boxes_are_not_vacuous_and_empty_clamps_are_empty(tally):
    """box <= K accepted + rim, rim being the points the widening by one index adds: K = 20 is the figure the feature was specified with,
    over all cases; what the helper achieves is 5.6 in 2D, 15.8 in 3D and 10.5 over all (half of the cells are slivers, needles or four
    random points)."""
    t2, t3 = tally[2], tally[3]
    assert t2["box"] <= 7 * t2["accepted"] + t2["rim"], t2
    assert t3["box"] <= 18 * t3["accepted"] + t3["rim"], t3
    assert t2["box"] + t3["box"] <= 12 * (t2["accepted"] + t3["accepted"]) + t2["rim"] + t3["rim"]
    assert t2["empty"] > 500 and t3["empty"] > 300                          # lattices beside the cell: every one of them an empty box
