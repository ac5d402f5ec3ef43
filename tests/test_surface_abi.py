"""CPU suite: the surface loads exist at every layer that can be seen without a GPU -- include/nsx.h declares the six entry points, the
enums and the totals, nsx.API lists them, the cross-compiled libnsx.so exports them and holds the kernels of csrc/nsx_surface.hip for gfx950,
and the Python class has the methods."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nsx_set_surface", "nsx_surface_info", "nsx_get_surface_layout", "nsx_compute_surface", "nsx_surface_field_components",
         "nsx_get_surface_field")
ENUMS = {"NSX_SURFACE_SYMMETRIC": 0, "NSX_SURFACE_GRADIENT": 1, "NSX_SURFACE_AT_FACES": 0, "NSX_SURFACE_AT_NODES": 1, "NSX_SURFACE_PRESSURE": 0}
ORDER = ("NSX_SURFACE_PRESSURE", "NSX_SURFACE_TRACTION", "NSX_SURFACE_SHEAR", "NSX_SURFACE_SHEAR_MAGNITUDE", "NSX_SURFACE_NORMAL",
         "NSX_SURFACE_YPLUS", "NSX_SURFACE_FIELD_COUNT")


def test_surface_entry_points_enums_kernels_and_methods_are_there():
    import __graft_entry__ as ge
    ge.build()                       # hipcc cross-compiles gfx950 without a GPU
    from navierstokes_project_nm4pde_amd import nsx, problem
    from navierstokes_project_nm4pde_amd._lib import DEV_SO
    text = open(os.path.join(ROOT, "include", "nsx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(DEV_SO)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*nsx_handle\s*\*" % name, header), name
        assert name in nsx.API
        assert hasattr(lib, name), name
        assert not re.search(r"\d", name)                               # tests/test_adaptor_header.py scans names without digits
    assert text.index("---- surface loads ----") > text.index("---- running statistics")
    assert text.index("---- surface loads ----") < text.index("---- measurement")
    for name, value in ENUMS.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(nsx, name[4:]) == value
    found = re.search(r"enum\s*\{\s*(NSX_SURFACE_PRESSURE[^}]*)\}", header).group(1)
    assert tuple(s.split("=")[0].strip() for s in found.split(",")) == ORDER   # consecutive from 0
    for k, name in enumerate(ORDER):
        assert getattr(nsx, name[4:]) == k
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*nsx_surface_totals\s*;", header).group(1)
    fields = re.findall(r"(double|int64_t)\s+(\w+)(?:\[(\d)\])?\s*;", struct)
    assert fields == [("double", "area", ""), ("double", "force_pressure", "3"), ("double", "force_viscous", "3"), ("double", "torque", "3"),
                      ("double", "flux", ""), ("double", "pressure_integral", ""), ("int64_t", "n_faces", "")]
    assert [f for f, _ in nsx.SurfaceTotals._fields_] == [f[1] for f in fields] and ctypes.sizeof(nsx.SurfaceTotals) == 8 * 13
    blob = open(DEV_SO, "rb").read()
    assert b"gfx950" in blob
    for kernel in (b"k_surface_faces", b"k_surface_nodes", b"k_surface_fold"):
        assert kernel in blob
    for method in ("set_surface", "surface_info", "surface_layout", "compute_surface", "surface_field"):
        assert callable(getattr(nsx.Nsx, method))
    assert callable(problem.boundary_faces)
    L = nsx.lib()
    counts = {"nsx_set_surface": 8, "nsx_surface_info": 2, "nsx_get_surface_layout": 5, "nsx_compute_surface": 2,
              "nsx_surface_field_components": 3, "nsx_get_surface_field": 4}
    for name, n in counts.items():
        assert len(getattr(L, name).argtypes) == n, name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == n, name


def test_boundary_faces_generalises_obstacle_faces():
    import numpy as np
    from conftest import Problem
    from navierstokes_project_nm4pde_amd.problem import boundary_faces, obstacle_faces
    for dim in (2, 3):
        p = Problem("cylinder", dim, 1)
        cells, lf, groups = boundary_faces(p.mesh)
        assert len(cells) == len(p.mesh.bface_ids) and sorted(set(groups.tolist())) == [0, 1, 2, 3]
        assert np.array_equal(groups, p.mesh.bface_ids)                 # the ids of the cylinder meshes are 0 .. 3: group = id
        oc, ol = obstacle_faces(p.mesh, 3)
        c3, l3, g3 = boundary_faces(p.mesh, [3])
        assert np.array_equal(c3, oc) and np.array_equal(l3, ol) and not g3.any()
        c, l, g = boundary_faces(p.mesh, [3, 0])
        assert set(g.tolist()) == {0, 1} and np.array_equal(c[g == 0], oc) and (g == 1).sum() == (p.mesh.bface_ids == 0).sum()
        assert len(set(zip(cells.tolist(), lf.tolist()))) == len(cells)  # no (cell, face) pair twice
