"""GPU suite: every path of the Schur-complement CG (csrc/nsx_cg.hip, cg() in csrc/nsx_solve.hip) DIRECTLY against an extended-precision
restatement of SolverCG (tests/cg_reference.py), through the test hook nsx_schur_cg -- the solve the preconditioners call, on the
caller's vectors.  A converged solve hides what is wrong in the iteration (CG corrects itself); here the iteration itself is pinned:

  iterates   rtol = 0, maxiter = k for k in (0, 1, 2, 3, 5, 8, 13, 21, 30): status 1 after exactly k steps, x_k entry by entry and res_k;
             k = 0 returns the guess bit for bit
  stopping   tolerances between two record lows of the reference's residuals (and the reference's own rtol = 1e-2): status 0 after
             EXACTLY the reference's steps, with the iterate of that step
  guesses    zero; a guess scaled with the solution, x_ref (1 + 0.5 xi) (a unit-size random guess is invisible: |S x0| / |b| < 1e-2);
             float64(x_ref): converged at step 0, x comes back bit for bit
  b = 0      steps 0, status 0, x all zeros
  state      the solves of a handle run back to back (mailbox ring, region swap, parity of the persistent kernel): after every one
             no fallback and no dirty mailbox word; a fallback ends the handle's cases with a failure

The data of the reference are the device's own negative_S_tilde, factors and block pointer (Nsx.schur(), Nsx.ilu(1)); the meshes are
the smallest on which each kernel can still go wrong: A = 3D level-1 cylinder (745 pressure rows of 14-76 entries: more than the 64
entries of four 16-lane chunks), B = 2D level-2 cylinder (366 rows of 6-22 entries: shorter than one chunk), C = 3D level-2 cylinder
(2485 rows).  Block layouts: uniform blocks of 96, 128, 129, 256, 257 rows plus the remainder, a ragged layout (blocks of 1, 2, 15, 16,
17, 31, 33, 64, 95, 96 rows, then 96-row blocks), the internal layout of the bench (8 virtual ranks, colour order, schur_max_rows 96: eight
blocks of 70-137 rows here; the reference then works in the internal numbering), 2-row blocks on C (1243 blocks: more than a resident grid and more than one
partial-sum array holds: k_cgd_fold) and 96-row blocks on C (up to 971 unique columns per block of at most 1024).

Every case asserts WHICH kernel ran: nsx_path_info (path, rows per lane group, operator in LDS, dense inverses, blocks per partial sum)
and the profile table (cg_S / cgd_A, cgd_B / spmv_S, cg_update, ilu_solve_S).  Environment that is read once per handle or per schedule
(NSX_CG_PERSISTENT, NSX_DENSE_S) gets a handle of its own; NSX_CG_PRES / NSX_CG_LRES / NSX_CG_FUSED are switched between the solves of
one handle.  Tolerances: K x (deviation of two float64 restatements from the reference + 4 eps), K measured -- see tests/cg_reference.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cg_reference as R
from conftest import Problem, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HANDLE_KEYS = ("NSX_CG_PERSISTENT", "NSX_DENSE_S")
SOLVE_KEYS = ("NSX_CG_PRES", "NSX_CG_LRES", "NSX_CG_FUSED")
CG_LPOOL, CG_MAXB, CG_MAX_WG, CGD_PARTS = 6656, 256, 1024, 1024   # limits of csrc/nsx_cg.hip the expected path follows from

MESHES = {"A": ("cylinder", 3, 1), "B": ("cylinder", 2, 2), "C": ("cylinder", 3, 2)}
_problems, _operators = {}, {}


def problem(mesh):
    if mesh not in _problems:
        _problems[mesh] = Problem(*MESHES[mesh])
    return _problems[mesh]


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2), time)


def blocks_of(layout, n):
    if layout == "ragged":
        return R.ragged_ptr(n)
    if layout == "internal":
        return None          # nsx_set_internal_layout builds them
    return R.block_ptr(n, int(layout))


def expected_path(op, handle_env, solve_env, comm):
    """the label of the kernel that has to run (cg_schur_persistent / cg_schur_fused / schur_cg restated)"""
    rows = int(np.max(np.diff(op.bptr)))
    nblk = len(op.bptr) - 1
    dense = handle_env.get("NSX_DENSE_S") != "0"
    persistent = handle_env.get("NSX_CG_PERSISTENT") != "0" and not comm and dense and rows <= CG_MAXB and nblk <= CG_MAX_WG
    if persistent:
        rpg = 0 if solve_env.get("NSX_CG_PRES") == "0" else 6 if rows <= 96 else 8 if rows <= 128 else 0
        nnz = int(np.max(op.rp[op.bptr[1:]] - op.rp[op.bptr[:-1]]))
        lres = rpg > 0 and solve_env.get("NSX_CG_LRES") != "0" and nnz <= CG_LPOOL
        return ("persistent", rpg, lres) if rpg else ("persistent", 0, False, "two register sets" if rows <= 128 else "one wide set")
    if solve_env.get("NSX_CG_FUSED") != "0" and dense and rows <= CG_MAXB:
        return ("two launches", "ncclAllReduce" if comm else "no communicator", "fold" if nblk > CGD_PARTS else "no fold")
    return ("launch per operation", "explicit inverses" if dense else "triangular solves")   # (ilu_solve applies them whatever the block size)


def observed_path(op, info, allreduces):
    """the label of the kernel that ran, from what the handle reports: nsx_path_info and the all-reduces the solve issued
    (nsx_comm_counters).  Which apply_P body k_cg_schur<0, false> took has no observable: "two register sets" / "one wide set" follows
    from the largest block's rows (nb <= 128 or not), as in the kernel."""
    rows = int(np.max(np.diff(op.bptr)))
    if info["schur_cg_path"] == 2:
        rpg, lres = info["schur_cg_rows_per_lane_group"], bool(info["schur_cg_operator_in_lds"])
        return ("persistent", rpg, lres) if rpg else ("persistent", 0, lres, "two register sets" if rows <= 128 else "one wide set")
    if info["schur_cg_path"] == 3:
        return ("two launches", "ncclAllReduce" if allreduces > 0 else "no communicator", "fold" if info["schur_blocks_per_partial"] > 1 else "no fold")
    return ("launch per operation", "explicit inverses" if info["schur_dense_inverses"] else "triangular solves")


SCOPES = {"persistent": ("cg_S",), "two launches": ("cgd_A", "cgd_B"), "launch per operation": ("spmv_S", "cg_update", "ilu_solve_S")}


def check_launches(path, table, steps):
    """the profile table of ONE solve: only the scopes of `path`, and as often as its algorithm launches them"""
    n = {k: table.get(k, {}).get("launches", 0) for names in SCOPES.values() for k in names}
    want = dict.fromkeys(n, 0)
    if path[0] == "persistent":
        want["cg_S"] = 1
    elif path[0] == "two launches":
        want["cgd_A"], want["cgd_B"] = steps + 1, steps    # the direction and product of the step after the last are speculative
    else:
        want["spmv_S"], want["cg_update"] = steps + 1, steps
        want["ilu_solve_S"] = steps + 1 if steps else 0    # h = P g_0, then one behind every update (the last one speculative)
    return [] if n == want else ["launches %s, expected %s" % (n, want)]


class Numbering:
    """caller's numbering <-> the numbering the device solves in (the identity without an internal layout)"""

    def __init__(self, perm=None):
        self.perm = perm

    def to_caller(self, v):
        return v if self.perm is None else np.ascontiguousarray(v[self.perm])

    def to_internal(self, v):
        if self.perm is None:
            return v
        out = np.empty_like(v)
        out[self.perm] = v
        return out


def make_handle(mesh, layout, comm):
    from navierstokes_project_nm4pde_amd import nsx
    p = problem(mesh)
    dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, nsx.COLOUR, 96) if layout == "internal" else None)
    try:
        ptr = blocks_of(layout, p.dofs.n_p)
        if ptr is not None:
            dev.set_schur_blocks(ptr)
        if comm:
            dev.comm_init_single()
        dev.set_solution(p.smooth_velocity())
        dev.assemble(nsx.TEMAM)
        dev.apply_boundary_values(*_bc(p, p.deltat))
        dev.prec_initialize(nsx.YOSIDA)
        S, (_, _, lu) = dev.schur(), dev.ilu(1)
        perm = None
        if layout == "internal":
            lay = dev.layout()
            perm, ptr = lay["pnode_perm"].astype(np.int64), lay["schur_ptr"]
            assert lay["on"] and len(ptr) - 1 == 8      # a virtual rank with more than 96 pressure rows stays a block of its own
        key = (mesh, layout)
        if key not in _operators:     # one reference per configuration; every other handle must hold the same numbers, bit for bit
            if perm is None:
                _operators[key] = R.Operator(S.indptr, S.indices, S.data, lu, ptr)
            else:
                rp, ci, sv = R.to_internal(S.indptr, S.indices, S.data, perm)
                _operators[key] = R.Operator(rp, ci, sv, R.to_internal(S.indptr, S.indices, lu, perm)[2], ptr)
        op = _operators[key]
        sv, luv = (S.data, lu) if perm is None else (R.to_internal(S.indptr, S.indices, S.data, perm)[2], R.to_internal(S.indptr, S.indices, lu, perm)[2])
        assert np.array_equal(op.sv, sv) and np.array_equal(op.lu, luv) and np.array_equal(op.bptr, ptr), "the handles of one configuration differ"
        return dev, op, Numbering(perm)
    except BaseException:
        dev.close()
        raise


def run_handle(mesh, layout, handle_env, solve_envs, want_paths, comm=False):
    """every call of R.schedule for every environment of `solve_envs`, back to back on ONE fresh handle created under `handle_env`;
    asserts at the end with every failure listed"""
    saved = {k: os.environ.pop(k, None) for k in HANDLE_KEYS + SOLVE_KEYS}
    os.environ.update(handle_env)
    failures, ran, worst = [], set(), {}
    dev = None
    try:
        dev, op, num = make_handle(mesh, layout, comm)
        refs = {g: R.reference(op, g) for g in R.GUESSES}
        b = R.rhs(op.n)
        calls = R.schedule(refs["zero"], refs["visible"], refs["exact"])
        for g in ("zero", "visible"):
            assert len(R.stops(refs[g])) >= 5, (mesh, layout, g)
        assert any(c[0] == "exact" for c in calls) or (mesh, layout) == ("C", 2), "float64(x_ref) is not converged for rtol = 1e-2"
        dev.profile(True)
        dead = False
        for solve_env in solve_envs:
            for k in SOLVE_KEYS:
                os.environ.pop(k, None)
            os.environ.update(solve_env)
            want = expected_path(op, handle_env, solve_env, comm)
            for kind, guess, rtol, maxiter, steps_ref in calls + [("zero rhs", "zero", 1e-2, 100000, 0)]:
                tag = "%s/%s %s %s%s: %s %s rtol=%.6g maxiter=%d" % (mesh, layout, handle_env, solve_env, " comm" if comm else "", kind, guess, rtol, maxiter)
                ref = refs[guess]
                dev.profile_reset()
                allreduces = dev.comm_counters()[0]
                x, steps, last, status = dev.schur_cg(num.to_caller(np.zeros(op.n) if kind == "zero rhs" else b), num.to_caller(ref.x0), rtol=rtol, maxiter=maxiter)
                allreduces = dev.comm_counters()[0] - allreduces
                table, info, state = dev.profile_table(), dev.path_info(), dev.persistent_state()
                out = (num.to_internal(x), steps, last, status)
                if kind == "iterate":
                    fails, ratios = R.check_iterate(ref, maxiter, out)
                elif kind == "zero rhs":
                    fails, ratios = R.check_zero_rhs(out), {}
                else:
                    fails, ratios = R.check_stop(ref, rtol, steps_ref, out)
                got = observed_path(op, info, allreduces)
                ran.add(got)
                if got != want:
                    fails.append("ran %s, expected %s (%s)" % (got, want, {k: info[k] for k in ("schur_cg_path", "schur_dense_inverses", "schur_blocks", "schur_blocks_per_partial")}))
                fails += check_launches(got, table, steps)
                if want[0] == "persistent" and not state["cg_persistent"]:
                    fails.append("the handle reports no persistent Schur CG")
                print("schur_cg_unit", tag, got, "steps", steps, {k: "%.3f" % v for k, v in ratios.items()}, fails)
                failures += ["%s: %s" % (tag, f) for f in fails]
                for q, v in ratios.items():
                    if v > worst.get((got, q), (-1.0, ""))[0]:
                        worst[(got, q)] = (v, tag)
                if state["fallbacks"] != 0 or state["dirty_mailbox_words"] != 0 or info["fallbacks"] != 0:
                    failures.append("%s: fallbacks %d, dirty mailbox words %d" % (tag, state["fallbacks"], state["dirty_mailbox_words"]))
                    dead = True   # a kernel that timed out has switched the handle to another path: nothing more to learn from it
                    break
            if dead:
                break
    finally:
        if dev is not None:
            dev.close()
        for k in HANDLE_KEYS + SOLVE_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    for (path, q), (v, tag) in sorted(worst.items(), key=str):
        record("schur_cg_unit", mesh=mesh, layout=str(layout), env=str(handle_env), comm=comm, path=str(path), quantity=q, max_ratio=v, at=tag)
    for p in want_paths:
        if p not in ran:
            failures.append("%s/%s %s: %s never ran (ran: %s)" % (mesh, layout, handle_env, p, sorted(ran, key=str)))
    assert not failures, "\n".join(failures[:40] + (["... %d more" % (len(failures) - 40)] if len(failures) > 40 else []))


DEFAULT, NO_LRES, NO_PRES, NO_FUSED = {}, {"NSX_CG_LRES": "0"}, {"NSX_CG_PRES": "0"}, {"NSX_CG_FUSED": "0"}
TWO_SETS, WIDE = ("persistent", 0, False, "two register sets"), ("persistent", 0, False, "one wide set")
TWO_LAUNCHES = ("two launches", "no communicator", "no fold")


def test_persistent_kernel_blocks_of_96_rows():
    """k_cg_schur<6, true>, <6, false> (NSX_CG_LRES=0) and <0, false> with two register sets (NSX_CG_PRES=0), switched on one handle"""
    run_handle("A", 96, {}, [DEFAULT, NO_LRES, NO_PRES, DEFAULT], [("persistent", 6, True), ("persistent", 6, False), TWO_SETS])


def test_persistent_kernel_blocks_of_128_rows():
    """k_cg_schur<8, true> (the largest block has 6340 entries of the 6656 the LDS pool holds), <8, false>, <0, false> with nb <= 128"""
    run_handle("A", 128, {}, [DEFAULT, NO_LRES, NO_PRES], [("persistent", 8, True), ("persistent", 8, False), TWO_SETS])


@pytest.mark.parametrize("size", [129, 256])
def test_persistent_kernel_streamed_inverses_one_wide_register_set(size):
    """k_cg_schur<0, false> with nb > 128: the first block size beyond the register-resident variants, and the largest"""
    run_handle("A", size, {}, [DEFAULT], [WIDE])


def test_persistent_kernel_ragged_blocks():
    """blocks of 1 ... 96 rows in one grid: block tails, one-row blocks, full blocks"""
    run_handle("A", "ragged", {}, [DEFAULT, NO_LRES, NO_PRES], [("persistent", 6, True), ("persistent", 6, False), TWO_SETS])


def test_persistent_kernel_short_rows():
    """mesh B: rows of 6-22 entries, shorter than one 16-lane chunk"""
    run_handle("B", 96, {}, [DEFAULT, NO_LRES], [("persistent", 6, True), ("persistent", 6, False)])


def test_persistent_kernel_internal_layout():
    """the bench's shape: 8 virtual ranks in colour order, merged into Schur blocks of at most 96 rows, vectors permuted on the way in
    and out.  On this mesh no two ranks fit one block and the ranks themselves have 70-137 pressure rows (a rank larger than the limit
    stays a block of its own), so the kernel is the one with streamed inverses in one wide register set, not <6, true>"""
    run_handle("A", "internal", {}, [DEFAULT], [WIDE])


def test_persistent_kernel_near_the_unique_column_limit():
    """mesh C in 96-row blocks: up to 971 of the 1024 unique columns a block may have"""
    run_handle("C", 96, {}, [DEFAULT], [("persistent", 6, True)])


@pytest.mark.parametrize("layout", [96, 256, "ragged"])
def test_two_launches_per_iteration(layout):
    """NSX_CG_PERSISTENT=0: k_cgd_init / k_cgd_A / k_cgd_B; on the 96-row blocks also the launch-per-operation solver with the explicit
    inverses (NSX_CG_FUSED=0), switched on the same handle"""
    run_handle("A", layout, {"NSX_CG_PERSISTENT": "0"}, [DEFAULT] + ([NO_FUSED, DEFAULT] if layout == 96 else []),
               [TWO_LAUNCHES] + ([("launch per operation", "explicit inverses")] if layout == 96 else []))


def test_two_launches_per_iteration_with_a_communicator():
    """the same with the partial sums through ncclAllReduce (1-rank RCCL communicator)"""
    run_handle("A", 96, {}, [DEFAULT], [("two launches", "ncclAllReduce", "no fold")], comm=True)


def test_two_launches_per_iteration_with_folded_partial_sums():
    """mesh C in 2-row blocks: 1243 blocks, more than a resident grid holds (no switch needed) and more than a partial-sum array has
    entries: k_cgd_fold adds them in pairs"""
    run_handle("C", 2, {}, [DEFAULT], [("two launches", "no communicator", "fold")])


def test_launch_per_operation_with_triangular_solves():
    """NSX_CG_PERSISTENT=0 NSX_CG_FUSED=0 NSX_DENSE_S=0: cg() with spmv_S, cg_update and the sparse ilu_solve_S"""
    run_handle("A", 96, {"NSX_CG_PERSISTENT": "0", "NSX_DENSE_S": "0"}, [NO_FUSED], [("launch per operation", "triangular solves")])


def test_launch_per_operation_because_a_block_is_too_large():
    """257-row blocks, no switch: neither the persistent nor the two-launch kernels serve them (the preconditioner is still applied
    through the explicit inverses, which ilu_solve uses up to 4096-row blocks)"""
    run_handle("A", 257, {}, [DEFAULT], [("launch per operation", "explicit inverses")])


# ---- two processes
DIST_ITERATES = (1, 2, 3, 5, 8, 13)


def test_two_processes_iterates(tmp_path):
    """(dim 3, level 1, world 2, n_sub 4, colour order, Schur blocks of two sub-ranks) over host callbacks: the iterates of the two-launch
    solver with k_cgd_pack -- the owner evaluates -h / beta d - h for its neighbours' ghosts -- against the reference built from a
    single-process handle with the same blocks"""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    world, n_sub, merge = 2, 4, 2
    mesh = Mesh.cylinder(3, 1).partition(world, n_sub)
    dofs, tables = DoFs(mesh, "colour"), Tables(3)
    dev = nsx.Nsx(dofs, tables, 1e-3, 2e-4)
    try:
        ptr = np.ascontiguousarray(dofs.owned_p_ptr[::merge])
        dev.set_schur_blocks(ptr)
        dev.set_solution(0.05 * np.random.default_rng(5).standard_normal(dofs.n_dofs))
        dev.assemble(nsx.TEMAM)
        dev.apply_boundary_values(*cylinder_boundary_values(dofs, InletVelocity(3, 2), 2e-4))
        dev.prec_initialize(nsx.YOSIDA)
        S, (_, _, lu) = dev.schur(), dev.ilu(1)
    finally:
        dev.close()
    op = R.Operator(S.indptr, S.indices, S.data, lu, ptr)
    refs = {g: R.reference(op, g) for g in ("zero", "visible")}
    inp, out = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, b=R.rhs(op.n), zero=refs["zero"].x0, visible=refs["visible"].x0, ks=np.array(DIST_ITERATES))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in HANDLE_KEYS + SOLVE_KEYS:
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29583", os.path.join(ROOT, "tests", "schur_cg_dist_worker.py"), str(n_sub), str(merge), str(inp), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    info = dict(zip(d["path_keys"], d["path_info"]))
    assert info["schur_cg_path"] == 3 and info["neighbours"] >= 1 and info["ghost_nodes"] > 0, info
    assert "cgd_A" in d["scopes"] and "cgd_B" in d["scopes"] and "spmv_S" not in d["scopes"] and "cg_S" not in d["scopes"], list(d["scopes"])
    failures, worst = [], {}
    for gi, guess in enumerate(("zero", "visible")):
        for ki, k in enumerate(DIST_ITERATES):
            steps, last, status = int(d["steps"][gi, ki]), float(d["last"][gi, ki]), int(d["status"][gi, ki])
            fails, ratios = R.check_iterate(refs[guess], k, (d["x"][gi, ki], steps, last, status), k_margin=R.K_DIST)
            print("schur_cg_unit two processes", guess, k, {q: "%.3f" % v for q, v in ratios.items()}, fails)
            failures += ["%s k=%d: %s" % (guess, k, f) for f in fails]
            for q, v in ratios.items():
                worst[q] = max(worst.get(q, 0.0), v)
    record("schur_cg_unit", mesh="A", layout="two processes x 4 sub-ranks, blocks of 2", path="two launches, host callbacks, k_cgd_pack",
           **{"max_ratio_" + q: v for q, v in worst.items()})
    assert not failures, "\n".join(failures)
