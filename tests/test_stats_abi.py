"""CPU suite: the running statistics exist at every layer that can be seen without a GPU -- include/nsx.h declares the five entry points under
"running statistics", nsx.API lists them, the cross-compiled libnsx.so exports them and holds the kernels of csrc/nsx_stats.hip for gfx950,
and the host front-end exports the writer the mirror's NSX_STATS uses."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nsx_stats_begin", "nsx_stats_accumulate", "nsx_stats_info", "nsx_stats_components", "nsx_stats_get")
QUANTITIES = ("MEAN_U", "COMOMENT_U", "STRESS_U", "RMS_U", "TKE", "MEAN_P", "COMOMENT_P", "VAR_P", "RMS_P", "QUANTITY_COUNT")


def test_stats_entry_points_and_kernels_are_there():
    import __graft_entry__ as ge
    ge.build()                       # hipcc cross-compiles gfx950 without a GPU
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd._lib import DEV_SO, HOST_SO
    text = open(os.path.join(ROOT, "include", "nsx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(DEV_SO)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*nsx_handle\s*\*" % name, header), name
        assert name in nsx.API
        assert hasattr(lib, name), name
    section = text[text.index("/* ---- running statistics ---- */"):text.index("/* ---- measurement ---- */")]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, section), name
    assert "W' = W + w" in section and "Errors:" in section                 # the recurrence and the errors are part of the header
    assert re.search(r"enum\s*\{\s*NSX_STATS_VELOCITY = 1, NSX_STATS_PRESSURE = 2\s*\}", header)
    m = re.search(r"enum\s*\{\s*NSX_STATS_MEAN_U = 0,([^}]*)\}", header)
    assert m and ["NSX_STATS_MEAN_U"] + [s.strip() for s in m.group(1).split(",")] == ["NSX_STATS_" + q for q in QUANTITIES]
    assert (nsx.STATS_VELOCITY, nsx.STATS_PRESSURE) == (1, 2)
    assert [getattr(nsx, "STATS_" + q) for q in QUANTITIES] == list(range(10))
    blob = open(DEV_SO, "rb").read()
    assert b"gfx950" in blob and b"k_stats_update" in blob and b"k_stats_finish" in blob
    for method in ("stats_begin", "stats_accumulate", "stats_info", "stats_get"):
        assert callable(getattr(nsx.Nsx, method))
    L = nsx.lib()
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [3, 3, 5, 3, 4]
    host_header = open(os.path.join(ROOT, "include", "nsx_host.h")).read()
    assert re.search(r"\bint\s+nsxh_write_vtu_stats\s*\(", host_header)
    assert hasattr(ctypes.CDLL(HOST_SO), "nsxh_write_vtu_stats")
