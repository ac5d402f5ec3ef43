"""GPU suite of the opt-in inner precision (include/nsx.h: nsx_set_inner_precision).  NSX_INNER_FP32 stores two value streams of the
inner solves on the velocity block as float -- F as every F->vmult inside a preconditioner's vmult reads it, and the off-diagonal
entries of ILU(0)(F) in the lane-owner solve stream -- and computes everything in double as before:

    FP32 mode  ==  the FP64 code run on (double)(float)value.

The first half pins that identity exactly (the bounds are the ones the project asserts for the same operations in double, because the
arithmetic is the same); the second half runs whole time steps: against the oracle at the bounds the double path is held to (the
linear system is unchanged, only the preconditioner's data is rounded) and against an FP64 device from the same state for the
iteration counts.  Tests need a real MI355X."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Problem, record, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (mesh, dim, level, ranks, node order, virtual ranks of nsx_set_internal_layout or 0): four cases of tests/test_gpu_parity.py CASES and
# one handle that keeps deal.II's first-touch numbering on one rank and lets libnsx lay the nodes out (the shape of bench.py's problem)
CASES = [("cylinder", 3, 1, 6, "first_touch", 0), ("cylinder", 3, 2, 24, "colour", 0), ("cylinder", 2, 2, 5, "first_touch", 0),
         ("cube", 3, 4, 3, "first_touch", 0), ("cylinder", 3, 1, 1, "first_touch", 8)]

# asserted agreement of (velocity, pressure) with the oracle after a full step at tol_abs = 1e-11 / inner_rtol = 1e-10 with the device in
# NSX_INNER_FP32: the bound of the double path, 1e-10 each (tests/test_gpu_parity.py TIGHT_BOUND); cases whose floor is higher would be
# listed here with the measured value and the reason.  None is.
TIGHT_BOUND_FP32 = {}


def _case_id(c):
    return "%s%dd-l%d-r%d-%s" % c[:5] + ("-layout%d" % c[5] if c[5] else "")


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import (EthierSteinmann, InletVelocity, cylinder_boundary_values,
                                                         ethier_boundary_values)
    if p.mesh.bface_ids.max() > 3:
        return ethier_boundary_values(p.dofs, EthierSteinmann(p.nu), time)
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2 if p.dim == 3 else 3), time)


class Setup:
    """One configuration: device handles in the caller's numbering (with or without an internal layout) and the oracle on the
    numbering the device works in (the caller's, or the layout's permutation of it)."""

    def __init__(self, case):
        from navierstokes_project_nm4pde_amd import nsx
        kind, dim, level, nsub, ordering, layout = case
        self.case, self.case_id, self.layout = case, _case_id(case), layout
        self.p = Problem(kind, dim, level, n_sub=nsub, nu=1e-2 if kind == "cube" else 1e-3, deltat=4e-4 if kind == "cube" else None, ordering=ordering)
        self.first_flags = nsx.TEMAM | (nsx.DOUBLE_CONVECTION if self.p.mesh.bface_ids.max() > 3 else 0)
        self.step_flags = nsx.TEMAM if (dim == 2 or self.p.mesh.bface_ids.max() > 3) else 0
        self.prec = nsx.YOSIDA if dim == 3 else nsx.ASIMPLE
        self.pd = None
        self.devs = []

    def device(self, precision=None):
        from navierstokes_project_nm4pde_amd import nsx
        p = self.p
        dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(self.layout, nsx.COLOUR, 0) if self.layout else None, inner_precision=precision)
        self.devs.append(dev)
        return dev

    def oracle(self, dev):
        import oracle
        from navierstokes_project_nm4pde_amd.frontend import PermutedDoFs
        p = self.p
        if not self.layout:
            return oracle.Oracle(p.dofs, p.tables, p.nu, p.deltat)
        lay = dev.layout()
        self.pd = PermutedDoFs(p.dofs, lay["node_perm"], lay["pnode_perm"], lay["u_ptr"], lay["p_ptr"])
        return oracle.Oracle(self.pd, p.tables, p.nu, p.deltat)

    # -- the same operation on a device (caller's numbering) or on the oracle (the device's internal numbering)
    def set_state(self, o, u):
        if hasattr(o, "set_solution"):
            o.set_solution(u)
        else:
            un = self.pd.to_new(u) if self.pd is not None else u
            o.solution[:] = un
            o.solution_owned[:] = un

    def apply_bc(self, o, time):
        bd, bv = _bc(self.p, time)
        if hasattr(o, "set_solution") or self.pd is None:
            o.apply_boundary_values(bd, bv)
        else:
            bn = self.pd.dof_map[bd]
            k = np.argsort(bn)
            o.apply_boundary_values(bn[k].astype(np.int32), np.asarray(bv)[k])

    def solution(self, o):
        if hasattr(o, "set_solution"):
            return o.solution_owned
        x = np.array(o.solution_owned)
        return self.pd.to_old(x) if self.pd is not None else x

    def assembled_device(self, precision=None, u=None):
        """a handle with the first assembly and its boundary values done, from the parity suite's smooth state"""
        dev = self.device(precision)
        self.set_state(dev, self.p.smooth_velocity() if u is None else u)
        dev.assemble(self.first_flags)
        self.apply_bc(dev, self.p.deltat)
        return dev

    def rank_blocks(self, dev):
        """(scalar node permutation caller -> internal or None, node ranges of the ranks the ILU(0) of F runs on)"""
        if self.layout:
            lay = dev.layout()
            return np.asarray(lay["node_perm"], dtype=np.int64), np.asarray(lay["u_ptr"], dtype=np.int32)
        d = self.p.dofs
        return None, (np.asarray(d.owned_u_ptr, dtype=np.int32) if d.n_subdomains > 1 else np.array([0, d.n_u // d.dim], dtype=np.int32))

    def close(self):
        for d in self.devs:
            d.close()
        self.devs = []


@pytest.fixture(params=CASES, ids=_case_id)
def setup(request):
    s = Setup(request.param)
    yield s
    s.close()


def _round_f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ exact emulation

def test_inner_F_product_is_the_double_product_on_values_rounded_to_float(setup):
    from navierstokes_project_nm4pde_amd import nsx
    s = setup
    dev = s.assembled_device(nsx.INNER_FP32)
    dev.prec_initialize(s.prec)
    rp, ci = s.p.dofs.reference_sparsity(0)
    n_u = s.p.dofs.n_u
    v64 = dev.export_block(0, 0)
    A64 = sp.csr_matrix((v64, ci, rp), shape=(n_u, n_u))
    A32 = sp.csr_matrix((_round_f32(v64), ci, rp), shape=(n_u, n_u))   # (cross-component slots are structural zeros: rounding them changes nothing)
    x = np.random.default_rng(7).standard_normal(n_u)
    y = dev.inner_F_vmult(x)
    info = dev.path_info()
    e32, e64 = rel_err(y, A32 @ x), rel_err(y, A64 @ x)
    record("inner_fp32_F_vmult", case=s.case_id, err_vs_rounded=e32, err_vs_double=e64, staged=info["spmv_lds_staged"], flag=info["inner_F_fp32"])
    print("%s: F product FP32 vs rounded %.3e, vs double %.3e, lds-staged %d" % (s.case_id, e32, e64, info["spmv_lds_staged"]))
    # which kernel the product takes is read from the handle: only the LDS-staged SpMV has a float twin, and the handle says which ran
    assert info["inner_F_fp32"] == info["spmv_lds_staged"]
    assert info["spmv_lds_staged"] == 1, "every case of this file is expected on the LDS-staged SpMV"
    assert e32 < 1e-13, e32          # the bound of the double product (tests/test_gpu_parity.py:88): same arithmetic
    assert e64 > 1e-10, e64          # the flag is live
    # the outer product (system_matrix.vmult) stays on the double values
    xb = np.random.default_rng(8).standard_normal(s.p.dofs.n_dofs)
    dev64 = s.assembled_device()
    assert np.array_equal(dev.system_vmult(xb), dev64.system_vmult(xb))
    # back to FP64: the double product, and the handle says so
    dev.set_inner_precision(nsx.INNER_FP64)
    with pytest.raises(nsx.NsxError):      # call order: the preconditioner has to be initialised again
        dev.inner_F_vmult(x)
    dev.prec_initialize(s.prec)
    y64 = dev.inner_F_vmult(x)
    assert dev.path_info()["inner_F_fp32"] == 0
    assert rel_err(y64, A64 @ x) < 1e-13
    dev64.prec_initialize(s.prec)
    assert np.array_equal(y64, dev64.inner_F_vmult(x))


def _internal_factor(rp, ci, lu, perm):
    """the scalar factor (caller's numbering) on the numbering the device factorised in: rows and columns through perm, columns sorted"""
    n = len(rp) - 1
    if perm is None:
        return np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32), np.asarray(lu, dtype=np.float64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    r2, c2 = perm[rows], perm[np.asarray(ci, dtype=np.int64)]
    k = np.lexsort((c2, r2))
    rp2 = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(r2, minlength=n), out=rp2[1:])
    return rp2, c2[k].astype(np.int32), np.asarray(lu, dtype=np.float64)[k]


def test_velocity_triangular_solves_are_the_double_solves_on_factors_rounded_to_float(setup):
    import oracle
    from navierstokes_project_nm4pde_amd import nsx
    s = setup
    dim = s.p.dim
    dev = s.assembled_device(nsx.INNER_FP32)
    dev.prec_initialize(s.prec)
    perm, bptr = s.rank_blocks(dev)
    rp, ci, lu = _internal_factor(*dev.ilu(0), perm)        # nsx_ilu_get: always the double factors
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    lu32 = _round_f32(lu)
    lu32[rows == ci] = lu[rows == ci]                        # the inverse pivots stay double
    # ... and they ARE the double factors: those of a handle that never left FP64, bit for bit
    dev64 = s.assembled_device()
    dev64.prec_initialize(s.prec)
    assert np.array_equal(dev.ilu(0)[2], dev64.ilu(0)[2])
    b = np.random.default_rng(5).standard_normal(s.p.dofs.n_u)
    z = dev.ilu_apply(0, b)
    used = dev.path_info()["ilu_F_fp32"]                      # which stream the solve read is the handle's word, not the test's assumption
    e32 = e64 = 0.0
    for c in range(dim):
        bc_ = b[c::dim]
        zc = z[c::dim]
        if perm is not None:
            bi = np.empty_like(bc_)
            bi[perm] = bc_
            bc_, zc = bi, None
        z32, z64 = oracle.ilu0_solve(rp, ci, lu32, bptr, bc_), oracle.ilu0_solve(rp, ci, lu, bptr, bc_)
        if perm is not None:
            z32, z64, zc = z32[perm], z64[perm], z[c::dim]
        e32, e64 = max(e32, rel_err(zc, z32)), max(e64, rel_err(zc, z64))
    record("inner_fp32_ilu_apply", case=s.case_id, err_vs_rounded=e32, err_vs_double=e64, flag=used)
    print("%s: ILU apply FP32 vs rounded %.3e, vs double %.3e, float stream %d" % (s.case_id, e32, e64, used))
    # every case of this file has rank blocks that fit the lane-owner stream (DESIGN.md section 5 quotes all five as float): the float
    # kernel must be what ran in each of them (a path without a float twin -- tested below on the levelled ILU -- would report 0)
    assert used == 1, "the velocity triangular solves of this case are expected on the lane-owner stream, read as float"
    assert e32 < 1e-11, e32      # the bound of the double solve (tests/test_gpu_levelled.py:70)
    assert e64 > 1e-10, e64      # the flag is live
    # the Schur factors and their solve are untouched by the mode
    bp = np.random.default_rng(6).standard_normal(s.p.dofs.n_p)
    assert np.array_equal(dev.ilu_apply(1, bp), dev64.ilu_apply(1, bp))
    assert np.array_equal(dev.ilu(1)[2], dev64.ilu(1)[2])
    # FP64 handle: the double stream
    z_d = dev64.ilu_apply(0, b)
    assert dev64.path_info()["ilu_F_fp32"] == 0
    assert not np.array_equal(z_d, z)


def test_path_info_tells_which_streams_were_float():
    from navierstokes_project_nm4pde_amd import nsx
    s = Setup(CASES[4])                               # internal layout: LDS-staged SpMV + lane-owner stream
    try:
        dev = s.assembled_device()
        st = dev.solve_time_step(s.prec)
        info = dev.path_info()
        assert st["status"] == 0 and info["inner_F_fp32"] == 0 and info["ilu_F_fp32"] == 0
        dev.set_inner_precision(nsx.INNER_FP32)
        with pytest.raises(nsx.NsxError) as e:        # a vmult between the switch and the next initialisation is the call-order error
            dev.prec_vmult(s.prec, np.ones(s.p.dofs.n_dofs))
        assert e.value.code == -1
        st = dev.solve_time_step(s.prec)
        info = dev.path_info()
        assert st["status"] == 0 and info["inner_F_fp32"] == 1 and info["ilu_F_fp32"] == 1, info
        assert info["sweep_with_ilu_inside"] == 0
        dev.set_inner_precision(nsx.INNER_FP64)
        st = dev.solve_time_step(s.prec)
        info = dev.path_info()
        assert st["status"] == 0 and info["inner_F_fp32"] == 0 and info["ilu_F_fp32"] == 0, info
    finally:
        s.close()


def test_fused_sweep_is_not_used_in_fp32(monkeypatch):
    """NSX_ILU_MGS=1 (the opt-in kernel with the triangular solves inside the Gram-Schmidt sweep) reads the double stream only: in
    NSX_INNER_FP32 the separate kernels run and the handle says so"""
    from navierstokes_project_nm4pde_amd import nsx
    monkeypatch.setenv("NSX_ILU_MGS", "1")
    s = Setup(CASES[4])
    try:
        dev = s.assembled_device(nsx.INNER_FP32)
        st = dev.solve_time_step(s.prec)
        info = dev.path_info()
        assert st["status"] == 0 and info["sweep_with_ilu_inside"] == 0 and info["inner_F_fp32"] == 1 and info["ilu_F_fp32"] == 1, info
    finally:
        s.close()


def test_levelled_ilu_keeps_its_double_factors_and_says_so(monkeypatch):
    """few large ranks: the level-per-launch triangular solves (the switch of tests/test_gpu_levelled.py) have no float twin"""
    from navierstokes_project_nm4pde_amd import nsx
    monkeypatch.setenv("NSX_LEVELLED_MIN", "64")
    s = Setup(("cylinder", 3, 1, 3, "colour", 0))
    try:
        dev, dev64 = s.assembled_device(nsx.INNER_FP32), s.assembled_device()
        st, st64 = dev.solve_time_step(s.prec, tol_abs=1e-11, inner_rtol=1e-10), dev64.solve_time_step(s.prec, tol_abs=1e-11, inner_rtol=1e-10)
        info = dev.path_info()
        assert st["status"] == 0 and st64["status"] == 0
        assert info["ilu_F_fp32"] == 0 and info["inner_F_fp32"] == info["spmv_lds_staged"], info
        b = np.random.default_rng(5).standard_normal(s.p.dofs.n_u)
        assert np.array_equal(dev.ilu_apply(0, b), dev64.ilu_apply(0, b))      # the double factors, through the same kernels
        assert dev.path_info()["ilu_F_fp32"] == 0
        assert rel_err(dev.solution_owned, dev64.solution_owned) < 1e-8
    finally:
        s.close()


def test_back_to_fp64_is_bitwise_the_handle_that_never_left_it(setup):
    from navierstokes_project_nm4pde_amd import nsx
    s = setup
    u = s.p.smooth_velocity()
    dev, ref = s.assembled_device(u=u), s.assembled_device(u=u)
    dev.set_inner_precision(nsx.INNER_FP32)
    dev.prec_initialize(s.prec)
    st32 = dev.solve_time_step(s.prec, tol_abs=1e-9, inner_rtol=1e-6)
    x32 = dev.solution_owned
    assert st32["status"] == 0
    # the same state again (the solve changed nothing but the solution vectors), now in FP64
    dev.set_solution(u)
    dev.set_inner_precision(nsx.INNER_FP64)
    dev.prec_initialize(s.prec)
    st64 = dev.solve_time_step(s.prec, tol_abs=1e-9, inner_rtol=1e-6)
    ref.set_solution(u)
    ref.prec_initialize(s.prec)
    str_ = ref.solve_time_step(s.prec, tol_abs=1e-9, inner_rtol=1e-6)
    assert st64["status"] == 0 and str_["status"] == 0
    for key in ("outer_iterations", "inner_F_iterations", "inner_S_iterations", "n_F_solves", "n_S_solves"):
        assert st64[key] == str_[key], key
    assert st64["final_residual"] == str_["final_residual"]
    assert np.array_equal(dev.solution_owned, ref.solution_owned)
    assert np.array_equal(dev.solution, ref.solution)
    assert not np.array_equal(x32, ref.solution_owned)       # (and the FP32 solve was another computation)


def test_unknown_precisions_are_argument_errors(monkeypatch):
    from navierstokes_project_nm4pde_amd import nsx
    p = Problem("cylinder", 2, 1)
    dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat)
    try:
        for bad in (7, -1, 2):
            with pytest.raises(nsx.NsxError) as e:
                dev.set_inner_precision(bad)
            assert e.value.code == -1
    finally:
        dev.close()
    L = nsx.lib()
    monkeypatch.setenv("NSX_INNER_PRECISION", "bogus")
    h = ctypes.c_void_p()
    prm = nsx.Params(2, 0, 1e-3, 1e-2)
    assert L.nsx_create(ctypes.byref(prm), ctypes.byref(h)) == -1 and not h.value
    assert b"NSX_INNER_PRECISION" in L.nsx_last_error(None)
    with pytest.raises(nsx.NsxError):
        nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat)
    # the two spellings it accepts set the handle's initial value
    for word, flag in (("fp32", 1), ("fp64", 0)):
        monkeypatch.setenv("NSX_INNER_PRECISION", word)
        s = Setup(CASES[4])
        try:
            dev = s.assembled_device()
            assert dev.solve_time_step(s.prec)["status"] == 0
            assert dev.path_info()["inner_F_fp32"] == flag and dev.path_info()["ilu_F_fp32"] == flag
        finally:
            s.close()


# ------------------------------------------------------------------------------------------------ end to end

def _march(s, prec, aliased_id):
    """two steps at tightened tolerances (FP32 device, FP64 device, oracle, each from its own previous solution), then one at the
    reference's own tolerances (the two devices)"""
    from navierstokes_project_nm4pde_amd import nsx
    p = s.p
    u = p.smooth_velocity()
    d32, d64 = s.assembled_device(nsx.INNER_FP32, u=u), s.assembled_device(u=u)
    ora = s.oracle(d32)
    s.set_state(ora, u)
    ora.assemble(s.first_flags)
    s.apply_bc(ora, p.deltat)
    t = p.deltat
    nu_ = p.dofs.n_u
    tol = 1e-10 if p.deltat == 1e-3 else 1e-11       # tests/test_gpu_parity.py:152
    for step in range(2):
        t += p.deltat
        for o in (d32, d64, ora):
            o.assemble_time_step(s.step_flags)
            s.apply_bc(o, t)
        s32 = d32.solve_time_step(prec, tol_abs=tol, inner_rtol=1e-10)
        s64 = d64.solve_time_step(prec, tol_abs=tol, inner_rtol=1e-10)
        so = ora.solve_time_step(prec, tol_abs=tol, inner_rtol=1e-10)
        assert s32["status"] == 0 and s64["status"] == 0 and so["status"] == 0
        info = d32.path_info()
        x32, x64, xo = s.solution(d32), s.solution(d64), s.solution(ora)
        err_u = np.abs(x32[:nu_] - xo[:nu_]).max() / np.abs(xo[:nu_]).max()
        err_p = np.abs(x32[nu_:] - xo[nu_:]).max() / np.abs(xo[nu_:]).max()
        err64_u = np.abs(x64[:nu_] - xo[:nu_]).max() / np.abs(xo[:nu_]).max()
        err64_p = np.abs(x64[nu_:] - xo[nu_:]).max() / np.abs(xo[nu_:]).max()
        counts = {k: (s32[k], s64[k], so[k]) for k in ("outer_iterations", "inner_F_iterations", "inner_S_iterations")}
        record("inner_fp32_steps_tight", case=aliased_id, prec=prec, step=step, err_u=err_u, err_p=err_p, err64_u=err64_u, err64_p=err64_p,
               F_float=info["inner_F_fp32"], ilu_float=info["ilu_F_fp32"], **{k: list(v) for k, v in counts.items()})
        print("%s prec %d step %d: FP32 vs oracle u %.3e p %.3e (FP64: %.3e %.3e); outer/F/S (fp32, fp64, oracle) %s; float F %d ILU %d"
              % (aliased_id, prec, step, err_u, err_p, err64_u, err64_p, [counts[k] for k in counts], info["inner_F_fp32"], info["ilu_F_fp32"]))
        assert info["inner_F_fp32"] == 1
        bound_u, bound_p = TIGHT_BOUND_FP32.get((p.kind, p.dim, prec), (1e-10, 1e-10))
        assert err_u < bound_u and err_p < bound_p, (err_u, err_p)
        # against the FP64 DEVICE from the same state (the parent's behaviour): the margin tests/test_gpu_parity.py:169 grants two
        # implementations of one algorithm -- rounding the preconditioner's data at 6e-8 does not move an inner solve to 1e-10 by more
        # (a CPU probe with SciPy's GMRES on the oracle's F and factors found identical inner counts at 1e-2 / 1e-6 / 1e-10)
        for key, (a, b, _) in counts.items():
            assert abs(a - b) <= max(2, 0.05 * b), (key, a, b)
    # once more at the reference's own tolerances (1e-4 / 1e-2), where a restart more or less moves the count by rounding alone: the
    # margins test_reference_tolerances_iteration_counts grants device against oracle (tests/test_gpu_parity.py:187-189)
    t += p.deltat
    for o in (d32, d64):
        o.assemble_time_step(s.step_flags)
        s.apply_bc(o, t)
    s32, s64 = d32.solve_time_step(prec, maxiter=500, check=False), d64.solve_time_step(prec, maxiter=500, check=False)
    x32, x64 = s.solution(d32), s.solution(d64)
    diff = np.abs(x32 - x64).max() / np.abs(x64).max()
    record("inner_fp32_reference_tolerances", case=aliased_id, prec=prec, diff=diff, outer=[s32["outer_iterations"], s64["outer_iterations"]],
           inner_F=[s32["inner_F_iterations"], s64["inner_F_iterations"]], inner_S=[s32["inner_S_iterations"], s64["inner_S_iterations"]])
    print("%s prec %d reference tolerances: outer %d / %d, inner F %d / %d, inner S %d / %d, solutions differ by %.3e"
          % (aliased_id, prec, s32["outer_iterations"], s64["outer_iterations"], s32["inner_F_iterations"], s64["inner_F_iterations"],
             s32["inner_S_iterations"], s64["inner_S_iterations"], diff))
    assert s32["status"] == 0 and s64["status"] == 0
    assert abs(s32["outer_iterations"] - s64["outer_iterations"]) <= max(2, 0.2 * s64["outer_iterations"])
    assert diff < 1e-3, diff


def test_time_steps_in_fp32_match_the_oracle_and_iterate_like_fp64(setup):
    """Yosida in 3D, aSIMPLE in 2D"""
    _march(setup, setup.prec, setup.case_id)


def test_ayosida_in_fp32_the_aliased_product():
    """aYosida's F->vmult(yu, yu) (Preconditioners.hpp:507) reads the float copy as well; it runs no inner solve on F"""
    from navierstokes_project_nm4pde_amd import nsx
    s = Setup(CASES[0])
    try:
        d = s.assembled_device(nsx.INNER_FP32)
        d64 = s.assembled_device()
        for o in (d, d64):
            o.prec_initialize(nsx.AYOSIDA)
        src = np.random.default_rng(11).standard_normal(s.p.dofs.n_dofs)
        y, _ = d.prec_vmult(nsx.AYOSIDA, src, inner_rtol=1e-11)
        info = d.path_info()
        y64, _ = d64.prec_vmult(nsx.AYOSIDA, src, inner_rtol=1e-11)
        assert info["inner_F_fp32"] == 1 and info["ilu_F_fp32"] == 0 and d64.path_info()["inner_F_fp32"] == 0, info
        e = rel_err(y, y64)
        record("inner_fp32_ayosida_vmult", case=s.case_id, diff=e)
        print("%s: aYosida vmult FP32 vs FP64 %.3e" % (s.case_id, e))
        assert e > 0, e            # not the double product
        _march(s, nsx.AYOSIDA, s.case_id + "-aYosida")
    finally:
        s.close()


def test_distributed_solve_in_fp32_equals_single_process_in_fp32(tmp_path):
    """built like tests/test_gpu_distributed.py::test_distributed_solve_equals_single_process (3D level 1, 2 processes on one card, 3
    sub-ranks each, Yosida), the mode reached through NSX_INNER_PRECISION.  tests/dist_worker.py keeps the path info of rank 0 only, and
    whether a rank streams float depends on ITS chunk table and ITS schedule: tests/inner_precision_dist_worker.py writes path info and
    profile scopes per rank and step, and every rank is asserted on."""
    dim, level, world, n_sub, prec, ordering = 3, 1, 2, 3, 0, "first_touch"
    prefix = str(tmp_path / "dist")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", NSX_INNER_PRECISION="fp32")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29578", os.path.join(ROOT, "tests", "inner_precision_dist_worker.py"), str(dim), str(level), str(n_sub), str(prec), prefix, ordering]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [np.load("%s_rank%d.npz" % (prefix, k)) for k in range(world)]
    for k, d in enumerate(ranks):
        assert int(d["rank"]) == k and int(d["world"]) == world
        scopes = list(d["scopes"])
        for step, row in enumerate(d["path_info"]):          # this rank's paths after each of its three solves
            info = dict(zip(d["path_keys"], (int(v) for v in row)))
            record("inner_fp32_distributed_paths", rank=k, step=step, F_float=info["inner_F_fp32"], ilu_float=info["ilu_F_fp32"],
                   chunks=info["spmv_chunks"], chunks_behind_halo=info["spmv_chunks_behind_halo"])
            assert info["inner_F_fp32"] == 1, (k, step, info)          # the float product ran on THIS rank
            assert info["ilu_F_fp32"] == 1, (k, step, info)            # ... and its triangular solves read the float stream
            assert info["spmv_lds_staged"] == 1 and 0 < info["spmv_chunks_behind_halo"] <= info["spmv_chunks"], (k, info)
            assert info["neighbours"] >= 1 and info["ghost_nodes"] > 0
        assert "spmv_F" in scopes and "spmv_F_if" in scopes and "halo_u_wait" in scopes and "F_to_f32" in scopes, (k, scopes)
        assert (d["iters"] == ranks[0]["iters"]).all()
    d = ranks[0]
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    mesh = Mesh.cylinder(dim, level).partition(world, n_sub)
    dofs, tables = DoFs(mesh, ordering), Tables(dim)
    dt = 2e-4
    dev = nsx.Nsx(dofs, tables, 1e-3, dt, inner_precision=nsx.INNER_FP32)
    try:
        dev.set_solution(d["u0"])
        inlet = InletVelocity(dim, 2)
        t = 0.0
        for step in range(3):
            t += dt
            if step == 0:
                dev.assemble(nsx.TEMAM)
            else:
                dev.assemble_time_step(0)
            dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, t))
            st = dev.solve_time_step(prec, tol_abs=1e-10, inner_rtol=1e-10)
            info = dev.path_info()
            assert info["inner_F_fp32"] == 1 and info["ilu_F_fp32"] == 1
            x = dev.solution_owned
            err = np.abs(x - d["sols"][step]).max() / np.abs(x).max()
            record("inner_fp32_distributed", step=step, err=err, outer=[st["outer_iterations"], int(d["iters"][step])])
            print("distributed FP32 step %d: workers vs one process %.3e, outer %d / %d" % (step, err, int(d["iters"][step]), st["outer_iterations"]))
            assert err < 1e-8, (step, err)                                    # tests/test_gpu_distributed.py:69
            assert abs(st["outer_iterations"] - int(d["iters"][step])) <= 1   # :71
    finally:
        dev.close()


def test_values_beyond_floats_range_fail_the_initialisation():
    """deltat = 1e-45 puts the entries of F = M / deltat + ... near 1e40: fine as doubles (the FP64 handle initialises its
    preconditioner), not finite as floats: in NSX_INNER_FP32 the initialisation fails with NSX_ERR_NUMERIC and a message instead of
    leaving an inf in the stream, and the handle works again once it is back in FP64"""
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    p = Problem("cylinder", 2, 1, n_sub=2, deltat=1e-45)
    devs = []
    try:
        for precision in (nsx.INNER_FP64, nsx.INNER_FP32):
            dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, inner_precision=precision)
            devs.append(dev)
            dev.set_solution(np.zeros(p.dofs.n_dofs))
            dev.assemble(nsx.TEMAM)
            dev.apply_boundary_values(*cylinder_boundary_values(p.dofs, InletVelocity(2, 3), 1e-2))
        d64, d32 = devs
        big = np.abs(d64.export_block(0, 0)).max()
        assert np.isfinite(big) and big > 3.5e38, big           # the premise: representable as double, not as float
        d64.prec_initialize(nsx.YOSIDA)
        assert np.isfinite(d64.ilu(0)[2]).all()
        with pytest.raises(nsx.NsxError) as e:
            d32.prec_initialize(nsx.YOSIDA)
        assert e.value.code == -5 and "float" in str(e.value), str(e.value)      # NSX_ERR_NUMERIC
        with pytest.raises(nsx.NsxError) as e:                  # nothing half-initialised is left usable
            d32.inner_F_vmult(np.ones(p.dofs.n_u))
        assert e.value.code == -1
        with pytest.raises(nsx.NsxError) as e:                  # the same through the solver's own initialisation
            d32.solve_time_step(nsx.YOSIDA)
        assert e.value.code == -5
        d32.set_inner_precision(nsx.INNER_FP64)
        d32.prec_initialize(nsx.YOSIDA)
        x = np.random.default_rng(2).standard_normal(p.dofs.n_u)
        assert np.array_equal(d32.inner_F_vmult(x), d64.inner_F_vmult(x))
    finally:
        for dev in devs:
            dev.close()
