"""CPU suite: tests/diagnostics_reference.py, the extended-precision restatement the GPU tests of the flow diagnostics compare the kernels
with, pinned against closed forms -- so that those tests do not rest on a restatement alone.

A quadratic velocity field is its own P2 interpolant, and the assembly's degree-5 rule integrates |u|^2 (degree 4), (div u)^2, |grad u|^2 and
|curl u|^2 (degree 2) exactly: on a box the helper has to reproduce a tensor Gauss-Legendre quadrature of the analytic integrands."""
import math

import numpy as np
import pytest

import diagnostics_reference as R

HI = {2: [1.0, 2.0], 3: [1.0, 2.0, 1.5]}
TOL = 1e-13


def _box(dim):
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    mesh = Mesh.box(dim, [3, 3, 2][:dim], hi=HI[dim])
    return mesh, DoFs(mesh), Tables(dim)


@pytest.mark.parametrize("dim", [2, 3])
def test_quadratic_field_integrals_match_closed_forms(dim):
    mesh, dofs, tables = _box(dim)
    u = R.interpolate_quadratic(dofs)
    res = R.flow_diagnostics(mesh, dofs, tables, u, np.zeros_like(u), 1e-2)
    t, ex = res["totals"], R.quadratic_closed_forms(HI[dim])
    assert ex["div2"] > 0.1 and ex["enstrophy"] > 0.1          # nothing degenerate is being compared
    for key, got in (("kinetic_energy", t["kinetic_energy"]), ("div2", t["div_l2"] ** 2), ("grad_l2_sq", t["grad_l2_sq"]),
                     ("enstrophy", t["enstrophy"]), ("volume", t["volume"])):
        assert abs(got - ex[key]) <= TOL * ex[key], (key, got, ex[key])
    # previous = 0: the change is the field itself
    assert abs(t["change_l2"] ** 2 - 2 * ex["kinetic_energy"]) <= TOL * 2 * ex["kinetic_energy"]
    assert t["n_cells"] == dofs.n_cells == res["cells"].shape[1]
    # previous = the field: no change, everything else as before
    same = R.flow_diagnostics(mesh, dofs, tables, u, u, 1e-2)
    assert same["totals"]["change_l2"] == 0.0 and same["totals"]["kinetic_energy"] == t["kinetic_energy"]
    # per-cell shares add up to the totals and every cell has its volume
    assert abs(math.fsum(res["cells"][R.DIV2]) - t["div_l2"] ** 2) <= TOL * ex["div2"]
    assert np.all(res["cells"][R.VOLUME] > 0)


@pytest.mark.parametrize("dim", [2, 3])
def test_constant_field_gives_cfl_and_speed_from_the_vertices(dim):
    mesh, dofs, tables = _box(dim)
    c = np.array([0.7, -1.3, 0.4][:dim])
    dt = 2.5e-2
    u = np.zeros(dofs.n_dofs)
    u[:dofs.n_u] = np.tile(c, dofs.n_u // dim)
    res = R.flow_diagnostics(mesh, dofs, tables, u, u, dt)
    # grad lambda_k of every cell straight from its vertices: lambda_k(x) = a_k + g_k . x with lambda_k(x_j) = delta_kj
    X = np.asarray(mesh.vertices)[np.asarray(mesh.cells)]
    M = np.concatenate([np.ones(X.shape[:2] + (1,)), X], axis=2)      # rows (1, x_j)
    grad = np.linalg.inv(M)[:, 1:, :]                                  # [nc][d][k]
    cfl_cells = dt * np.abs(np.einsum("d,cdk->ck", c, grad)).max(axis=1)
    assert np.allclose(res["cells"][R.CFL], cfl_cells, rtol=1e-12, atol=0)
    t = res["totals"]
    assert abs(t["cfl_max"] - cfl_cells.max()) <= 1e-12 * cfl_cells.max()
    speed = float(np.sqrt(c @ c))
    assert abs(t["speed_max"] - speed) <= TOL * speed and np.allclose(res["cells"][R.SPEED], speed, rtol=TOL, atol=0)
    vol = float(np.prod(HI[dim]))
    assert abs(t["volume"] - vol) <= TOL * vol
    assert abs(t["kinetic_energy"] - 0.5 * speed ** 2 * vol) <= TOL * 0.5 * speed ** 2 * vol
    # a constant field has no gradient: what is left is rounding of the shape-function gradients' partition of zero
    assert t["grad_l2_sq"] <= 1e-26 * speed ** 2 * vol and t["change_l2"] == 0.0
