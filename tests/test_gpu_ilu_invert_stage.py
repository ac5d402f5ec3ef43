"""GPU suite: the block inverses of the Schur ILU(0) built with the factor's in-block entries staged in LDS (k_ilu_invert_lds<true>,
NSX_ILU_INVERT_STAGE=1: the default) against the same kernel reading the factor from global memory (=0) and against k_ilu_invert
(NSX_ILU_INVERT_LDS=0): the factors and ilu_apply(1, b) bit for bit, on one handle, every initialisation rebuilding.

Block tables on the Schur matrix of the 3D level-1 cylinder (745 rows) as tests/test_gpu_ilu.py forces them: 96 rows, exactly 112 (the
last size k_ilu_invert_lds takes), 113 (k_ilu_invert), ragged (empty blocks, blocks of 1 .. 65 rows); and on a 4 x 4 x 4 box (125
pressure rows) one block of 112 rows, about the densest a mesh of the front-end gives (32 % full: 142 KB staged; the cylinder's: 18 %).  Whether the staged variant ran
(nsx_ilu_invert_staged) must be what the LDS arithmetic says:
    rows^2 * 8 + entries * 8 + round_up(entries * 2, 8) + 900 (the two static tables)  <=  limit,
rows / entries of the largest block / of the block with most in-block entries, limit = the device's 160 KiB, or NSX_LDS_OPTIN where
that is lower.  These blocks stay below the 50 % at which a 112-row block no longer fits beside its 98 KB matrix, so the fallback is
reached through that knob: at a limit of exactly the bytes needed the block is staged, one byte below it is not.
nsx_ilu_path_info must not see any of this."""
import os

import numpy as np
import pytest

import ilu_reference as R
from conftest import Problem

pytestmark = pytest.mark.gpu

KEYS = ("NSX_ILU_INVERT_STAGE", "NSX_ILU_INVERT_LDS", "NSX_LDS_OPTIN", "NSX_SCHUR_CACHE")
LDS_DEVICE = 160 * 1024          # MI355X: dynamic LDS a workgroup may opt in to
STATIC_TABLES = (113 + 112) * 4
MESHES = {"A": ("cylinder", 3, 1, {}), "box444": ("box", 3, 1, {"n": [4, 4, 4]})}
_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _handles_closed_and_environment_restored():
    saved = {k: os.environ.get(k) for k in KEYS}
    yield
    for dev, _ in _handles.values():
        dev.close()
    _handles.clear()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def set_env(**env):
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ["NSX_SCHUR_CACHE"] = "0"
    os.environ.update({k: str(v) for k, v in env.items()})


def handle(mesh):
    from navierstokes_project_nm4pde_amd import nsx
    if mesh not in _handles:
        kind, dim, level, kw = MESHES[mesh]
        p = Problem(kind, dim, level, **kw)
        dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat)
        try:
            dev.set_solution(p.smooth_velocity())
            dev.assemble(nsx.TEMAM)
            if kind == "cylinder":
                from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
                dev.apply_boundary_values(*cylinder_boundary_values(p.dofs, InletVelocity(dim, 2), p.deltat))
            else:
                bd = np.sort(p.dofs.boundary_dofs(0)).astype(np.int32)
                dev.apply_boundary_values(bd, np.linspace(0.5, 1.5, len(bd)))
            n2 = dev.n_u // dim
            fptr = R.block_ptr(n2, 85)
            dev.set_ranks(fptr, np.round(fptr.astype(np.float64) * dev.n_p / n2).astype(np.int32))
        except BaseException:
            dev.close()
            raise
        _handles[mesh] = (dev, np.random.default_rng(3).standard_normal(dev.n_p))
    return _handles[mesh]


def lds_needed(S, ptr):
    """(bytes the staged kernel needs, rows of the largest block, most in-block entries of a block) from the graph and the blocks"""
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    blk = np.searchsorted(ptr, np.arange(S.shape[0]), side="right") - 1
    inside = (S.indices >= ptr[blk[rows]]) & (S.indices < ptr[blk[rows] + 1])
    per_block = np.bincount(blk[rows][inside], minlength=len(ptr) - 1)
    n, nz = int(np.max(np.diff(ptr))), int(per_block.max())
    return n * n * 8 + nz * 8 + ((nz * 2 + 7) & ~7) + STATIC_TABLES, n, nz


def build(dev, b, **env):
    from navierstokes_project_nm4pde_amd import nsx
    set_env(**env)
    dev.prec_initialize(nsx.YOSIDA)
    return dev.ilu(1)[2].copy(), dev.ilu_apply(1, b), dev.ilu_invert_staged(1), dev.ilu_path_info(1)


CASES = [("A", 96), ("A", 112), ("A", 113), ("A", "ragged"), ("box444", 112)]


@pytest.mark.parametrize("mesh,layout", CASES, ids=["%s-%s" % c for c in CASES])
def test_staged_inverses_equal_the_unstaged_ones_and_the_hook_follows_the_lds_arithmetic(mesh, layout):
    dev, b = handle(mesh)
    n = dev.n_p
    ptr = R.ragged_ptr(n, 96) if layout == "ragged" else R.block_ptr(n, layout)
    dev.set_schur_blocks(ptr)
    lu1, x1, staged1, path1 = build(dev, b)                                   # the default: staging on
    need, rows, nz = lds_needed(dev.schur(), ptr)
    in_lds = rows <= 112
    print("%s %s: largest block %d rows, most in-block entries %d (%.0f %% of a dense block), %d bytes of LDS staged" %
          (mesh, layout, rows, nz, 100.0 * nz / (rows * rows), need))
    assert rows == min(n, 96 if layout == "ragged" else layout)
    assert path1["invert"] == ("lds" if in_lds else "global") and path1["max_block_rows"] == rows and path1["max_block_nnz"] == nz
    assert staged1 == (in_lds and need <= LDS_DEVICE)
    if layout in (96, "ragged"):
        assert staged1                                                        # blocks of up to 96 rows (the flagship's) fit the device
    runs = {"stage 0": build(dev, b, NSX_ILU_INVERT_STAGE=0), "stage 1": build(dev, b, NSX_ILU_INVERT_STAGE=1),
            "invert in global memory": build(dev, b, NSX_ILU_INVERT_LDS=0)}
    if in_lds:                                                                # the fallback at the edge of the arithmetic
        runs["limit = need"] = build(dev, b, NSX_LDS_OPTIN=need)
        runs["limit = need - 1"] = build(dev, b, NSX_LDS_OPTIN=need - 1)
        runs["limit above the device's"] = build(dev, b, NSX_LDS_OPTIN=1 << 30)
    want_staged = {"stage 0": False, "stage 1": staged1, "invert in global memory": False, "limit = need": need <= LDS_DEVICE, "limit = need - 1": False,
                   "limit above the device's": staged1}
    for name, (lu, x, staged, path) in runs.items():
        assert staged == want_staged[name], (name, staged)
        assert np.array_equal(lu, lu1), name
        assert np.array_equal(x, x1), "%s: ilu_apply(1, b) differs in %d entries" % (name, int(np.sum(x != x1)))
        if name == "invert in global memory":
            assert path["invert"] == "global" and {k: v for k, v in path.items() if k != "invert"} == {k: v for k, v in path1.items() if k != "invert"}
        else:
            assert path == path1, (name, path, path1)                         # nsx_ilu_path_info does not see the staging
    assert np.all(np.isfinite(x1)) and np.any(x1 != 0.0)


def test_the_112_row_block_falls_back_where_96_row_blocks_are_staged():
    """one limit between the two sizes: what a device with less LDS would do"""
    dev, b = handle("A")
    n = dev.n_p
    got = {}
    for layout in (96, 112):
        ptr = R.block_ptr(n, layout)
        dev.set_schur_blocks(ptr)
        ref = build(dev, b, NSX_ILU_INVERT_STAGE=0)
        got[layout] = (lds_needed(dev.schur(), ptr)[0], ref)
    limit = min((got[96][0] + got[112][0]) // 2, LDS_DEVICE)
    assert got[96][0] <= limit < got[112][0]
    for layout, staged_expected in ((96, True), (112, False)):
        dev.set_schur_blocks(R.block_ptr(n, layout))
        lu, x, staged, path = build(dev, b, NSX_LDS_OPTIN=limit)
        assert staged == staged_expected and path["invert"] == "lds", (layout, staged, path)
        assert np.array_equal(lu, got[layout][1][0]) and np.array_equal(x, got[layout][1][1])
