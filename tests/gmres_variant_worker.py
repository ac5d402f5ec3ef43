"""Handles and the variant schedule of tests/test_gpu_gmres.py, and -- run as a program -- ONE leg of its variants test in a fresh
process: gmres() reads NSX_AHEAD_MODE, NSX_AHEAD_MARGIN and NSX_ILU_MGS once per process (function-local statics), so every setting
needs a process of its own (like the *_dist_worker.py files).

    python tests/gmres_variant_worker.py OUT.npz      with the leg's settings in the environment

runs `schedule` and stores every solve's x, steps, status and last_residual, plus which sweep scopes ran."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

# name: (kind, dim, level, n_sub).  "A8": the rank table of 8 subdomains (the weak preconditioner); a trailing "i": the internal layout
# (8, COLOUR, 96); a trailing "f": NSX_INNER_FP32
MESHES = {"A": ("cylinder", 3, 1, 1), "B": ("cylinder", 2, 2, 1), "A8": ("cylinder", 3, 1, 8), "Ai": ("cylinder", 3, 1, 1), "A8f": ("cylinder", 3, 1, 8)}


def _bc(p, time):
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    return cylinder_boundary_values(p.dofs, InletVelocity(p.dim, 2), time)


def make_handle(name):
    """(name, problem, initialised handle, the Schur system as a cg_reference.Operator in the numbering the solve runs in; .perm: caller's
    pressure node -> that numbering, or None)"""
    import cg_reference as C
    from conftest import Problem
    from navierstokes_project_nm4pde_amd import nsx
    kind, dim, level, n_sub = MESHES[name]
    p = Problem(kind, dim, level, n_sub=n_sub, ordering="colour" if n_sub > 1 else "first_touch")
    internal, fp32 = name.endswith("i"), name.endswith("f")
    dev = nsx.Nsx(p.dofs, p.tables, p.nu, p.deltat, layout=(8, nsx.COLOUR, 96) if internal else None,
                  inner_precision=nsx.INNER_FP32 if fp32 else None)
    try:
        if n_sub > 1:
            ptr = np.asarray(p.dofs.owned_p_ptr)          # the rank table's pressure ranges are the Schur blocks
        else:
            ptr = C.block_ptr(p.dofs.n_p, 96)
            if not internal:
                dev.set_schur_blocks(ptr)
        dev.set_solution(p.smooth_velocity())
        dev.assemble(nsx.TEMAM)
        dev.apply_boundary_values(*_bc(p, p.deltat))
        dev.prec_initialize(nsx.YOSIDA)
        S, (_, _, lu) = dev.schur(), dev.ilu(1)
        if internal:      # the solve runs in the handle's own numbering: the reference too
            lay = dev.layout()
            perm, ptr = lay["pnode_perm"].astype(np.int64), lay["schur_ptr"]
            assert lay["on"]
            rp, ci, sv = C.to_internal(S.indptr, S.indices, S.data, perm)
            op = C.Operator(rp, ci, sv, C.to_internal(S.indptr, S.indices, lu, perm)[2], ptr)
            op.perm = perm
        else:
            op = C.Operator(S.indptr, S.indices, S.data, lu, ptr)
            op.perm = None
        return name, p, dev, op
    except BaseException:
        dev.close()
        raise


def schur_solve(dev, op, mode, b, x0, **kw):
    """nsx_gmres on the Schur system with b, x0 and the returned x in the numbering of `op` (the caller's, or the internal layout's)"""
    from navierstokes_project_nm4pde_amd import nsx
    if op.perm is None:
        return dev.gmres(nsx.GMRES_S, mode, b, x0, **kw)
    out = dev.gmres(nsx.GMRES_S, mode, np.ascontiguousarray(b[op.perm]), np.ascontiguousarray(x0[op.perm]), **kw)
    x = np.empty_like(out["x"])
    x[op.perm] = out["x"]
    out["x"] = x
    return out


VARIANT_ITERATES = (0, 5, 8, 28, 29, 57)
VARIANT_MESHES = ("B", "A8", "Ai")


def schedule(get):
    """the solves every leg of the variants test runs: {label: solve}, and the profile table of the velocity solves.  Schur system of the
    2D mesh: pinned iterates from zero and the nearly invariant case; velocity system in the rank-table and the internal layout: a
    solve to 1e-14 from zero (a second cycle) in the plain, the zero and the fused-zero mode, and plain / fused from a guess."""
    import gmres_reference as G
    from navierstokes_project_nm4pde_amd import nsx
    out, scopes = {}, {}
    _, _, dev, op = get("B")
    b = G.rhs(op.n)
    for k in VARIANT_ITERATES:
        out["B iterate %d" % k] = schur_solve(dev, op, nsx.GMRES_PLAIN, b, np.zeros(op.n), tol=0.0, maxiter=k, abs_tol=True)
    br = G.nearly_invariant_rhs(op)
    for k in (5, 8):
        out["B reorth %d" % k] = schur_solve(dev, op, nsx.GMRES_PLAIN, br, np.zeros(op.n), tol=0.0, maxiter=k, abs_tol=True)
    for name in ("A8", "Ai"):
        _, p, dev, _ = get(name)
        n = p.dofs.n_u
        rng = np.random.default_rng([G.SEED, n])
        b, y = rng.standard_normal(n), rng.standard_normal(n)
        dev.profile(True)
        dev.profile_reset()
        plain = dev.gmres(nsx.GMRES_F, nsx.GMRES_PLAIN, b, None, tol=1e-14, maxiter=400)
        t = dev.profile_table()
        dev.profile(False)
        scopes[name] = {k: t.get(k, {}).get("launches", 0) for k in ("mgs_sweep", "ilu_mgs", "add_and_dot", "ilu_solve_F", "axpy_multi")}
        out[name + " plain"] = plain
        if name == "A8":      # pinned iterates of the system that has a reference (gmres_reference.velocity_reference): before and behind the restart
            for k in (5, 29):
                out["A8 velocity iterate %d" % k] = dev.gmres(nsx.GMRES_F, nsx.GMRES_PLAIN, G.rhs(n), None, tol=0.0, maxiter=k, abs_tol=True)
        out[name + " zero"] = dev.gmres(nsx.GMRES_F, nsx.GMRES_ZERO, b, None, tol=1e-14, maxiter=400)
        out[name + " fused zero"] = dev.gmres(nsx.GMRES_F, nsx.GMRES_FUSED_ZERO_NEG, b, y, tol=1e-14, maxiter=400, neg_out=y)
        x0 = plain["x"] * (1 + 0.5 * rng.standard_normal(n))
        out[name + " guess plain"] = dev.gmres(nsx.GMRES_F, nsx.GMRES_PLAIN, b, x0, tol=1e-6, maxiter=400)
        out[name + " guess from"] = dev.gmres(nsx.GMRES_F, nsx.GMRES_FUSED_FROM_X0, b, x0, tol=1e-6, maxiter=400)
        st = dev.persistent_state()
        assert st["fallbacks"] == 0 and st["dirty_mailbox_words"] == 0, (name, st)
    return out, scopes


def main(path):
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_handle(name)
        return made[name]
    try:
        out, scopes = schedule(get)
    finally:
        for _, _, dev, _ in made.values():
            dev.close()
    flat = {}
    for label, s in out.items():
        flat[label + "|x"] = s["x"]
        flat[label + "|meta"] = np.array([s["steps"], s["status"], s["last_residual"]], dtype=np.float64)
    for name, t in scopes.items():
        flat[name + "|scopes"] = np.array([t[k] for k in sorted(t)], dtype=np.float64)
    np.savez(path, **flat)


if __name__ == "__main__":
    main(sys.argv[1])
