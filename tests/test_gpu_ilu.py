"""GPU suite: every factorisation, inversion and solve kernel of the block-Jacobi ILU(0) (csrc/nsx_ilu.hip, csrc/nsx_ilu_lanes.hpp)
DIRECTLY against an extended-precision restatement (tests/ilu_reference.py), entry by entry.

A case = set the environment, nsx_set_ranks / nsx_set_schur_blocks, nsx_prec_initialize, then
  factors   Nsx.ilu(which) against `factor` in long double on the device's own matrix (F's scalar entries from export_block(0, 0), the
            Schur matrix from Nsx.schur()), each entry measured against its absolute-term sum; entries outside the blocks exactly 0.0
  solves    Nsx.ilu_apply(which, b) against `solve` in long double on the DEVICE's factors, entry by entry relative to max |x| of the
            block, for a seeded normal vector, unit vectors at the first and last row of the first, a middle and the last block, and
            b = 0 (exactly 0 back)
  path      nsx_ilu_path_info: the factorisation, inversion and solve kernel that ran, E, PF, ncomp, float stream, the schedule's sizes

Meshes, the smallest that reach every path: A = 3D level-1 cylinder (F: 4806 P2 rows of 10-75 entries, NCOMP 3; S: 745 rows),
B = 2D level-2 cylinder (F: 1364 rows of 6-22 entries, NCOMP 2; S: 366 rows).  The lane-owner stream runs in all its instantiations
NCOMP x E x PF x double / float on layouts whose sweeps -- checked on the host from the stream's slab counts before anything runs --
take every exit of the sweep loop (slab counts = 0, 4, 8, 12 mod 16, and an empty sweep).  The last test asserts that every reachable
instantiation ran.  Tolerances: K x (deviation of two float64 restatements from the reference + 4 eps), K measured -- see
tests/ilu_reference.py."""
import hashlib
import os

import numpy as np
import pytest

import cg_reference as CG
import ilu_reference as R
from conftest import Problem, record

pytestmark = pytest.mark.gpu

MESHES = {"A": ("cylinder", 3, 1), "B": ("cylinder", 2, 2)}
ENV_KEYS = ("NSX_ILU_EPT", "NSX_PF", "NSX_BPW_F", "NSX_BPW_S", "NSX_DENSE_S", "NSX_ILU_SMALL", "NSX_ILU_FACTOR_LDS", "NSX_ILU_INVERT_LDS",
            "NSX_LEVELLED_MIN", "NSX_DENSE_MAX", "NSX_ILU_MGS")
# limits of csrc/nsx_ilu.hip / csrc/nsx_setup.hip the expected kernels follow from
ILU_WAVES, ILU_DENSE_ROWS, FACTOR_LDS_MAX, INVERT_LDS_ROWS, LEVELLED_MIN, LANES_K = 4, 512, 80 * 1024, 112, 4096, 12

_state = {"handles": {}, "refs": {}, "factors": {}, "solves": {}}
RAN = set()          # every kernel instantiation some case has asserted from nsx_ilu_path_info
RATIOS = {}          # kernel -> largest error / (err64 + 4 eps)


@pytest.fixture(scope="module", autouse=True)
def _handles_closed_and_environment_restored():
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    yield
    for dev in [h["dev"] for h in _state["handles"].values()]:
        dev.close()
    for v in _state.values():
        v.clear()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2), time)


def set_env(env):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})


def handle(mesh, internal=False, env=None):
    """one assembled handle per (mesh, layout kind, schedule environment of an internal layout): the matrices never change, the block
    tables and the environment do.  Returns a dict: dev, dim, the scalar graph and values of F in the caller's numbering."""
    from navierstokes_project_nm4pde_amd import nsx
    key = (mesh, internal, tuple(sorted((env or {}).items())) if internal else ())
    if key not in _state["handles"]:
        if internal:
            set_env(env or {})      # an internal layout builds its blocks itself: the schedule's environment is read with the first initialise
        p = Problem(*MESHES[mesh])
        dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, nsx.COLOUR, 96) if internal else None)
        try:
            dev.set_solution(p.smooth_velocity())
            dev.assemble(nsx.TEMAM)
            dev.apply_boundary_values(*_bc(p, p.deltat))
            g0 = p.dofs.reference_sparsity(0)
            rows = np.repeat(np.arange(len(g0[0]) - 1), np.diff(g0[0]))
            sel = (rows % p.dim == 0) & (np.asarray(g0[1]) % p.dim == 0)       # same-component entries carry the scalar F
            rp, ci = dev.scalar_graph(0)
            assert sel.sum() == len(ci) and np.array_equal(np.asarray(g0[1])[sel] // p.dim, ci)
            _state["handles"][key] = {"dev": dev, "p": p, "dim": p.dim, "F": (rp, ci, dev.export_block(0, 0)[sel].copy())}
        except BaseException:
            dev.close()
            raise
    return _state["handles"][key]


def lds_bytes(g):
    """ilu_factor_lds_bytes(rows of the largest block, most in-block entries of a block), restated"""
    cnt = np.concatenate([[0], np.cumsum(np.add.reduceat(g.inside.astype(np.int64), g.rp[:-1]))])
    nz = max(int(cnt[b] - cnt[a]) for a, b in R._blocks(g.bptr))
    rows = int(np.max(np.diff(g.bptr)))
    return ((nz + 3) & ~3) * 10 + (rows + 4) * 2 * (4 + ILU_WAVES), rows, nz


def expected_kernels(g, which, ncomp, env, stream_ok):
    """(factorisation, inversion, solve) as ilu_factor / ilu_solve choose them, restated from the graph, the blocks and the environment"""
    nbytes, rows, nz = lds_bytes(g)
    levelled = rows > int(env.get("NSX_LEVELLED_MIN", LEVELLED_MIN))
    dense = which == 1 and str(env.get("NSX_DENSE_S", 1)) != "0" and not levelled and rows <= 4096 and ncomp == 1 and \
        (rows <= 256 or int(np.sum(np.diff(g.bptr).astype(np.int64) ** 2)) <= 32 << 20)
    if levelled:
        factor = "level"
    elif str(env.get("NSX_ILU_FACTOR_LDS", 1)) != "0" and rows <= 4096 and nz < 65535 and nbytes <= FACTOR_LDS_MAX:
        factor = "lds"
    elif str(env.get("NSX_ILU_SMALL", 1)) != "0" and rows <= ILU_DENSE_ROWS:
        factor = "dense_row"
    else:
        factor = "general"
    invert = None if not dense else "lds" if str(env.get("NSX_ILU_INVERT_LDS", 1)) != "0" and rows <= INVERT_LDS_ROWS else "global"
    if levelled:
        solve = "levelled"
    elif dense and rows * 8 <= 48 * 1024:
        solve = "dense"
    elif stream_ok and (rows + 64) * 8 * ncomp <= 65536:
        solve = "lanes"
    else:
        solve = "block_lds" if rows * ncomp * 8 <= 65536 else "block_global"
    return factor, invert, solve


def stream_of(g, which, ncomp, env, n_blocks):
    """the lane-owner stream's statistics for this case as the device library builds it (host/ilu_stream.hpp through the host hook),
    or None where a wave's rows do not fit the stream's 16-bit addresses"""
    from navierstokes_project_nm4pde_amd.frontend import ilu_stream_stats
    key = "NSX_BPW_F" if which == 0 else "NSX_BPW_S"
    bpw = int(env[key]) if key in env else max(1, min(64, int(680.0 * n_blocks / max(1, g.n) + 0.5)))
    if (int(np.max(np.diff(g.bptr))) + 64) * 8 * ncomp > 65536:
        return None
    try:
        return ilu_stream_stats(g.rp, g.ci, g.bptr, bpw, ncomp, 2, int(env.get("NSX_ILU_EPT", 2)))
    except ValueError:
        return None


def sweep_classes(st):
    """which exits of the sweep loop (csrc/nsx_ilu_lanes.hpp) the stream's sweeps take: slab count modulo 16, "empty" for no slab"""
    counts = st["fwd_slabs"] + st["bwd_slabs"]
    assert all(c % 4 == 0 for c in counts)
    return {"empty" if c == 0 else c % 16 for c in counts}


def _cached(kind, key, make):
    if key not in _state[kind]:
        _state[kind][key] = make()
    return _state[kind][key]


def run_case(mesh, which, ptr, env=None, fp32=False, pfs=(8,), internal=False, want=None, tag=""):
    """one case (see the module's docstring); returns (nsx_ilu_path_info after the last solve, the stream's statistics or None).
    ptr: block table in rows of the matrix (None with the internal layout).  want: (factorisation, inversion, solve) kernel the case
    is ABOUT -- asserted beside the restated choice."""
    from navierstokes_project_nm4pde_amd import nsx
    env = dict(env or {})
    h = handle(mesh, internal, env)
    dev, dim = h["dev"], h["dim"]
    ncomp = dim if which == 0 else 1
    set_env(env)
    n2, n_p = dev.n_u // dim, dev.n_p
    perm = None
    if internal:
        lay = dev.layout()
        perm = (lay["node_perm"] if which == 0 else lay["pnode_perm"]).astype(np.int64)
        ptr = np.asarray(lay["u_ptr"] if which == 0 else lay["schur_ptr"])
        n_blocks_dev = len(ptr) - 1
    else:
        ptr = np.asarray(ptr, dtype=np.int32)
        if which == 0:
            dev.set_ranks(ptr, np.round(ptr.astype(np.float64) * n_p / n2).astype(np.int32))
            dev.set_schur_blocks(R.block_ptr(n_p, 96))
        else:
            fptr = R.block_ptr(n2, 85)
            dev.set_ranks(fptr, np.round(fptr.astype(np.float64) * n_p / n2).astype(np.int32))
            dev.set_schur_blocks(ptr)
        n_blocks_dev = len(ptr) - 1
    dev.set_inner_precision(nsx.INNER_FP32 if fp32 else nsx.INNER_FP64)
    dev.prec_initialize(nsx.YOSIDA)
    # ---- the matrix and the factors, in the numbering the blocks live in
    if which == 0:
        rp, ci, a = h["F"]
    else:
        S = dev.schur()
        rp, ci, a = S.indptr, S.indices, S.data
    rpd, cid, lu = dev.ilu(which)
    assert np.array_equal(rp, rpd) and np.array_equal(ci, cid)
    if perm is not None:
        (rp_i, ci_i, a), lu = CG.to_internal(rp, ci, a, perm), CG.to_internal(rp, ci, lu, perm)[2]
        rp, ci = rp_i, ci_i
    layout_key = (mesh, which, internal, np.asarray(ptr).tobytes())
    ref = _cached("refs", layout_key + (hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest(),), lambda: R.FactorReference(rp, ci, a, ptr))
    g = ref.g
    st = stream_of(g, which, ncomp, env, n_blocks_dev)
    kernels = expected_kernels(g, which, ncomp, env, st is not None)
    if want is not None:
        assert kernels == tuple(want), (tag, kernels, want)        # the case reaches the kernel it is about
    failures = []
    f, ratio = R.compare_factor(ref, lu)
    print("%s factor %s: error / (err64 + 4 eps) = %.3f, err64 %.3e, bound %.3e" % (tag, kernels[0], ratio, ref.err64, ref.bound()))
    failures += ["%s factor: %s" % (tag, m) for m in f]
    info = dev.ilu_path_info(which)
    if (info["factor"], info["invert"]) != kernels[:2]:
        failures.append("%s: factorisation / inversion kernel %s, expected %s" % (tag, (info["factor"], info["invert"]), kernels[:2]))
    nbytes, rows, nz = lds_bytes(g)
    if (info["blocks"], info["max_block_rows"], info["max_block_nnz"]) != (n_blocks_dev, rows, nz) or info["factor_lds_bytes"] != (nbytes if kernels[0] == "lds" else 0):
        failures.append("%s: schedule %s, expected %d blocks, %d rows, %d entries, %d bytes" % (tag, info, n_blocks_dev, rows, nz, nbytes))
    RAN.add(("factor", kernels[0]) + (("more than 64 KiB",) if kernels[0] == "lds" and nbytes > 65536 else ()))
    if kernels[1]:
        RAN.add(("invert", kernels[1]))
    RATIOS[("factor", kernels[0])] = max(RATIOS.get(("factor", kernels[0]), 0.0), ratio)
    record("ilu_unit", case=tag, kind="factor", kernel=kernels[0], ratio=ratio, err64=ref.err64, bound=ref.bound())
    if kernels[1]:
        record("ilu_unit", case=tag, kind="invert", kernel=kernels[1])
    # ---- the solves, on the device's own factors
    lu_key = hashlib.sha1(np.ascontiguousarray(lu).tobytes()).hexdigest()
    f32_stream = fp32 and which == 0 and kernels[2] == "lanes"
    factors = _cached("factors", layout_key + (lu_key, f32_stream), lambda: R.Factors(g, lu, f32_stream))
    vectors = [("normal", R.rhs(g.n, ncomp))]
    for r in R.unit_rhs_rows(ptr):
        e = np.zeros(g.n * ncomp)
        e[r * ncomp + r % ncomp] = 1.0
        vectors.append(("unit %d" % r, e))
    vectors.append(("zero", np.zeros(g.n * ncomp)))

    def to_caller(v):
        return v if perm is None else np.ascontiguousarray(v.reshape(g.n, ncomp)[perm].reshape(-1))

    def to_internal(v):
        if perm is None:
            return v
        out = np.empty((g.n, ncomp))
        out[perm] = v.reshape(g.n, ncomp)
        return out.reshape(-1)

    for pf in pfs:
        os.environ["NSX_PF"] = str(pf)
        worst, loosest = 0.0, 0.0
        for name, b in vectors:
            x = to_internal(dev.ilu_apply(which, to_caller(b)))
            info = dev.ilu_path_info(which)
            got = (info["solve"], info["ncomp"])
            if kernels[2] == "lanes":
                got += (info["entries_per_tick"], info["slabs_per_set"], info["float_stream"], info["waves"], info["max_wave_rows"])
                expect = ("lanes", ncomp, int(env.get("NSX_ILU_EPT", 2)), pf, int(f32_stream), st["waves"], st["max_wave_rows"])
            else:
                expect = (kernels[2], ncomp)
            if got != expect:
                failures.append("%s PF %d %s: solve path %s, expected %s" % (tag, pf, name, got, expect))
            if name == "zero":
                if np.any(x != 0.0):
                    failures.append("%s PF %d: b = 0 does not give x = 0" % (tag, pf))
                continue
            sref = _cached("solves", layout_key + (lu_key, f32_stream, name), lambda: R.SolveReference(g, lu, b, ncomp, factors=factors))
            f, ratio = R.compare_solve(sref, x)
            failures += ["%s PF %d %s: %s" % (tag, pf, name, m) for m in f]
            worst, loosest = max(worst, ratio), max(loosest, sref.bound())
        kernel = ("lanes", ncomp, int(env.get("NSX_ILU_EPT", 2)), pf, "float" if f32_stream else "double") if kernels[2] == "lanes" else (kernels[2], ncomp)
        RAN.add(("solve",) + kernel)
        if kernels[2] == "lanes":
            if st["max_wave_rows"] > 64 * LANES_K:
                RAN.add(("lanes rows per wave", "more than %d" % (64 * LANES_K * (2 if st["max_wave_rows"] > 128 * LANES_K else 1))))
            for c in sweep_classes(st):
                RAN.add(("lanes sweep", ncomp, int(env.get("NSX_ILU_EPT", 2)), pf, c))
        RATIOS[("solve",) + kernel[:2]] = max(RATIOS.get(("solve",) + kernel[:2], 0.0), worst)
        print("%s solve %s: error / (err64 + 4 eps) = %.3f, largest bound %.3e" % (tag, kernel, worst, loosest))
        record("ilu_unit", case=tag, kind="solve", kernel="/".join(str(k) for k in kernel), ratio=worst, bound=loosest)
    assert not failures, "\n".join(failures)
    return info, st


_problems = {}


def _n(mesh, which):
    """rows of F's scalar graph (P2 nodes) / of the Schur matrix"""
    if mesh not in _problems:
        _problems[mesh] = Problem(*MESHES[mesh])
    p = _problems[mesh]
    return p.dofs.n_u // p.dim if which == 0 else p.dofs.n_p


# ------------------------------------------------------------------------------------------------------------------ F: layouts
@pytest.mark.parametrize("mesh", ["A", "B"])
def test_diagonal_blocks(mesh):
    """every block one row: no slab at all, x = b / d"""
    n = _n(mesh, 0)
    info, st = run_case(mesh, 0, np.arange(n + 1), want=("lds", None, "lanes"), tag="%s/F diagonal" % mesh)
    assert st["slabs"] == 0 and sweep_classes(st) == {"empty"}


@pytest.mark.parametrize("mesh", ["A", "B"])
def test_ragged_blocks(mesh):
    """an empty block in front, in the middle and at the end, blocks of 1, 2, 15, 16, 17, 63, 64, 65 rows, then 85-row blocks"""
    ptr = R.ragged_ptr(_n(mesh, 0))
    assert ptr[0] == ptr[1] and ptr[-1] == ptr[-2] and np.any(np.diff(ptr)[1:-1] == 0)
    run_case(mesh, 0, ptr, want=("lds", None, "lanes"), tag="%s/F ragged" % mesh)


# staged bytes of the LDS factorisation on A (ilu_factor_lds_bytes of the largest block): 320 rows below 64 KiB, 350 between 64 and
# 80 KiB (the attribute raise; 400 rows are still 80 944 < 81 920), 512 above -> a dense row per wave, 513 -> the general kernel
FACTOR_CASES = [(320, {}, 62704, "lds"), (350, {}, 69584, "lds"), (400, {}, 80944, "lds"), (512, {}, 107736, "dense_row"), (513, {}, 108032, "general"),
                (320, {"NSX_ILU_FACTOR_LDS": 0}, 62704, "dense_row"), (512, {"NSX_ILU_FACTOR_LDS": 0}, 107736, "dense_row"),
                (512, {"NSX_ILU_SMALL": 0}, 107736, "general")]


@pytest.mark.parametrize("rows,env,nbytes,kernel", FACTOR_CASES, ids=["%d-%s%s" % (c[0], c[3], "".join("-%s=%s" % kv for kv in c[1].items())) for c in FACTOR_CASES])
def test_factorisation_kernels_at_their_thresholds(rows, env, nbytes, kernel):
    n = _n("A", 0)
    ptr = R.block_ptr(n, rows)
    h = handle("A")
    got = lds_bytes(R.Graph(h["F"][0], h["F"][1], ptr))
    assert got[0] == nbytes and got[1] == rows, got                 # the figures the thresholds are aimed with, recomputed from the graph
    assert (nbytes <= 65536) == (rows == 320) and (nbytes <= FACTOR_LDS_MAX) == (rows <= 400)
    run_case("A", 0, ptr, env=env, want=(kernel, None, "lanes"), tag="A/F %d-row blocks %s" % (rows, env or ""))


@pytest.mark.parametrize("bpw,rows", [(10, 850), (19, 1615)])
def test_waves_of_more_than_768_and_1536_rows(bpw, rows):
    """the second and third trip of the load / scale / store passes of k_ilu_solve_lanes (64 x LANES_K rows per trip)"""
    info, st = run_case("A", 0, R.block_ptr(_n("A", 0), 85), env={"NSX_BPW_F": bpw}, pfs=(8, 4), want=("lds", None, "lanes"), tag="A/F 85-row blocks, %d per wave" % bpw)
    assert st["max_wave_rows"] == rows == info["max_wave_rows"] and rows > 64 * LANES_K * (1 if bpw == 10 else 2)


# the boundaries of the solve kernels on A (NCOMP 3), the remainder as a second block: (2666 + 64) x 24 bytes = 65 520 is the largest
# block the stream addresses; 2730 x 24 = 65 520 the largest whose x fits 64 KiB of LDS
SOLVE_CASES = [(2666, {}, "general", "lanes"), (2667, {}, "general", "block_lds"), (2730, {}, "general", "block_lds"),
               (2731, {}, "general", "block_global"), (4096, {}, "general", "block_global"), (4806, {}, "level", "levelled")]


@pytest.mark.parametrize("rows,env,factor,solve", SOLVE_CASES, ids=["%d-%s" % (c[0], c[3]) for c in SOLVE_CASES])
def test_solve_kernels_at_their_thresholds(rows, env, factor, solve):
    n = _n("A", 0)
    assert n == 4806
    run_case("A", 0, R.split_ptr(n, rows), env=env, want=(factor, None, solve), tag="A/F blocks of %d + %d rows" % (rows, n - rows))


@pytest.mark.parametrize("mesh", ["A", "B"])
def test_levelled_kernels_on_the_ragged_layout(mesh):
    """NSX_LEVELLED_MIN = 64: the 65- and 85-row blocks put the whole schedule on the level-per-launch kernels, empty blocks included"""
    run_case(mesh, 0, R.ragged_ptr(_n(mesh, 0)), env={"NSX_LEVELLED_MIN": 64}, want=("level", None, "levelled"), tag="%s/F ragged, levelled" % mesh)
    run_case(mesh, 1, R.ragged_ptr(_n(mesh, 1), 96), env={"NSX_LEVELLED_MIN": 64}, want=("level", None, "levelled"), tag="%s/S ragged, levelled" % mesh)


# ------------------------------------------------------------------------------------------------------------------ the stream matrix
STREAM_ENV = {"NSX_BPW_F": 1, "NSX_BPW_S": 1}     # one block per wave: the ragged layouts then have sweeps of every class (checked below)


def _stream_family(ncomp):
    """(mesh, which, block table) of the layouts the stream matrix of one NCOMP runs on"""
    if ncomp == 1:
        return [("A", 1, R.ragged_ptr(_n("A", 1), 96))]
    mesh = "A" if ncomp == 3 else "B"
    return [(mesh, 0, R.ragged_ptr(_n(mesh, 0)))]


@pytest.mark.parametrize("ncomp", [1, 2, 3])
def test_stream_layouts_take_every_exit_of_the_sweep_loop(ncomp):
    """host arithmetic on the device's own graphs, before anything runs: for every E the sweeps of the family's layouts have slab
    counts = 0, 4, 8 and 12 (mod 16) -- the exits NSX_USE(B), NSX_USE_HALF(A), NSX_USE(A), NSX_USE_HALF(B) -- and an empty sweep"""
    for mesh, which, ptr in _stream_family(ncomp):
        h = handle(mesh)
        if which == 0:
            rp, ci = h["F"][:2]
        else:
            rp, ci = h["dev"].scalar_graph(1)
        g = R.Graph(rp, ci, ptr)
        for ept in (1, 2, 3, 4):
            st = stream_of(g, which, ncomp, dict(STREAM_ENV, NSX_ILU_EPT=ept), len(ptr) - 1)
            assert sweep_classes(st) == {0, 4, 8, 12, "empty"}, (mesh, which, ept, sweep_classes(st))


@pytest.mark.parametrize("ept", [1, 2, 3, 4])
def test_stream_ncomp2_every_instantiation(ept):
    """B, NCOMP 2: E x PF 4 / 8 x double / float stream on the ragged layout and on the internal layout (8 virtual ranks in colour
    order; the reference works in the internal numbering)"""
    env = dict(STREAM_ENV, NSX_ILU_EPT=ept)
    for fp32 in (False, True):
        run_case("B", 0, R.ragged_ptr(_n("B", 0)), env=env, fp32=fp32, pfs=(8, 4), want=("lds", None, "lanes"), tag="B/F ragged E %d%s" % (ept, " float" if fp32 else ""))
        run_case("B", 0, None, env={"NSX_ILU_EPT": ept}, fp32=fp32, pfs=(8, 4), internal=True, want=("lds", None, "lanes"),
                 tag="B/F internal layout E %d%s" % (ept, " float" if fp32 else ""))


@pytest.mark.parametrize("ept", [1, 2, 3, 4])
def test_stream_ncomp3_every_instantiation(ept):
    """A, NCOMP 3: E x PF 4 / 8 with the double and with the float stream"""
    env = dict(STREAM_ENV, NSX_ILU_EPT=ept)
    for fp32 in (False, True):
        run_case("A", 0, R.ragged_ptr(_n("A", 0)), env=env, fp32=fp32, pfs=(8, 4), want=("lds", None, "lanes"), tag="A/F ragged E %d%s" % (ept, " float" if fp32 else ""))


@pytest.mark.parametrize("ept", [1, 2, 3, 4])
def test_stream_ncomp1_every_instantiation(ept):
    """the Schur matrix of A without explicit inverses (NSX_DENSE_S = 0), NCOMP 1: E x PF 4 / 8"""
    env = dict(STREAM_ENV, NSX_ILU_EPT=ept, NSX_DENSE_S=0)
    run_case("A", 1, R.ragged_ptr(_n("A", 1), 96), env=env, pfs=(8, 4), want=("lds", None, "lanes"), tag="A/S ragged sparse E %d" % ept)


# ------------------------------------------------------------------------------------------------------------------ S: layouts
S_CASES = [(96, {}, "lds"), (112, {}, "lds"), (113, {}, "global"), (256, {}, "global"), ("ragged", {}, "lds"), (96, {"NSX_ILU_INVERT_LDS": 0}, "global")]


@pytest.mark.parametrize("mesh", ["A", "B"])
@pytest.mark.parametrize("layout,env,invert", S_CASES, ids=["%s-%s%s" % (c[0], c[2], "".join("-%s=%s" % kv for kv in c[1].items())) for c in S_CASES])
def test_schur_blocks_with_explicit_inverses(mesh, layout, env, invert):
    """dense by default: k_ilu_invert_lds up to 112 rows, k_ilu_invert above, k_ilu_apply_dense for the solve"""
    n = _n(mesh, 1)
    ptr = R.ragged_ptr(n, 96) if layout == "ragged" else R.block_ptr(n, layout)
    run_case(mesh, 1, ptr, env=env, want=("lds", invert, "dense"), tag="%s/S %s%s" % (mesh, layout, " " + str(env) if env else ""))


def test_schur_matrix_as_one_sparse_block():
    """745 rows in one block without explicit inverses: the general factorisation kernel feeds the NCOMP 1 stream (one wave)"""
    run_case("A", 1, R.block_ptr(_n("A", 1), 745), env={"NSX_DENSE_S": 0}, want=("general", None, "lanes"), tag="A/S one block sparse")


# ------------------------------------------------------------------------------------------------------------------ summary
def test_every_reachable_instantiation_ran():
    """Runs last: over the cases above every factorisation, inversion and solve kernel and every instantiation of the stream kernel has
    been asserted from nsx_ilu_path_info, and every sweep-length class of every stream instantiation.  NOT reachable on these meshes
    (and at the sizes a GPU test can afford):
      k_ilu_solve_lanes_f32<1, E, PF>   only F has a float stream (nsx_ilu_apply(1) and the Schur CG read the double factors), and F has NCOMP 2 or 3
      k_ilu_solve<1, 8, true / false>   NCOMP 1 leaves the stream only with a wave above 8128 rows ((rows + 64) x 8 > 64 KiB)
      k_ilu_solve<2, 8, true>           needs a 2D block above 4032 rows ((rows + 64) x 16 > 64 KiB); B has 1364
      k_ilu_solve<2, 8, false>          needs 2 x 8 x rows > 64 KiB, i.e. 4097 rows and more: at the default threshold those are levelled
    The largest ratios error / (err64 + 4 eps) per kernel are printed and recorded ("ilu_unit"): K of tests/ilu_reference.py is 10 x
    the largest, rounded up."""
    for key in sorted(RATIOS, key=str):
        print("largest ratio %s: %.3f" % (key, RATIOS[key]))
        record("ilu_unit", case="summary", kind="largest ratio", kernel="/".join(str(k) for k in key), ratio=RATIOS[key])
    want = {("factor", "level"), ("factor", "lds"), ("factor", "lds", "more than 64 KiB"), ("factor", "dense_row"), ("factor", "general"),
            ("invert", "lds"), ("invert", "global"),
            ("solve", "levelled", 1), ("solve", "levelled", 2), ("solve", "levelled", 3), ("solve", "dense", 1),
            ("solve", "block_lds", 3), ("solve", "block_global", 3),
            ("lanes rows per wave", "more than 768"), ("lanes rows per wave", "more than 1536")}
    for ncomp in (1, 2, 3):
        for ept in (1, 2, 3, 4):
            for pf in (4, 8):
                kinds = ("double",) if ncomp == 1 else ("double", "float")
                want |= {("solve", "lanes", ncomp, ept, pf, k) for k in kinds}
                want |= {("lanes sweep", ncomp, ept, pf, c) for c in (0, 4, 8, 12, "empty")}
    missing = sorted(want - RAN, key=str)
    assert not missing, missing
