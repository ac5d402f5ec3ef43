"""CPU suite: the nodal fields exist at every layer that can be seen without a GPU -- include/nsx.h declares the three entry points and the
enum, nsx.API lists them, the cross-compiled libnsx.so exports them and holds the kernel of csrc/nsx_nodal.hip for gfx950, and the host
library exports the writer."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nsx_compute_nodal_fields", "nsx_nodal_field_components", "nsx_get_nodal_field")
ENUMS = {"NSX_FIELD_GRADIENT": 0, "NSX_FIELD_VORTICITY": 1, "NSX_FIELD_Q": 2, "NSX_FIELD_STRAIN": 3, "NSX_FIELD_DIVERGENCE": 4, "NSX_FIELD_COUNT": 5}


def test_nodal_field_entry_points_enums_kernel_and_writer_are_there():
    import __graft_entry__ as ge
    ge.build()                       # hipcc cross-compiles gfx950 without a GPU
    from navierstokes_project_nm4pde_amd import frontend, nsx
    from navierstokes_project_nm4pde_amd._lib import DEV_SO, HOST_SO
    text = open(os.path.join(ROOT, "include", "nsx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(DEV_SO)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*nsx_handle\s*\*" % name, header), name
        assert name in nsx.API
        assert hasattr(lib, name), name
        assert not re.search(r"\d", name)                               # tests/test_adaptor_header.py scans names without digits
    assert "nodal fields" in text and text.index("---- nodal fields") > text.index("---- tracer particles")
    for name, value in ENUMS.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(nsx, name[4:]) == value
    blob = open(DEV_SO, "rb").read()
    assert b"gfx950" in blob and b"k_nodal_fields" in blob
    for method in ("compute_nodal_fields", "nodal_field"):
        assert callable(getattr(nsx.Nsx, method))
    L = nsx.lib()
    assert len(L.nsx_compute_nodal_fields.argtypes) == 1 and len(L.nsx_nodal_field_components.argtypes) == 3
    assert len(L.nsx_get_nodal_field.argtypes) == 3
    # the writer of the host library
    host_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsx_host.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+nsxh_write_vtu_fields\s*\(", host_header)
    assert hasattr(ctypes.CDLL(HOST_SO), "nsxh_write_vtu_fields")
    assert callable(getattr(frontend.DoFs, "write_vtu_fields"))
