"""CPU suite: pins tests/surface_reference.py (the restatement the GPU tests of the surface loads compare the kernels with) by closed forms on
the box meshes with ALL boundary faces, and checks the derived bound of the totals -- (C1 + fold depth) 2^-53 A, surface_reference's
docstring -- for the plain float64 run against the long double run on every mesh the GPU tests use.

The state is probe_reference.quadratic_state: the quadratic velocity of diagnostics_reference plus p = 7 + g . x, g = (2, -1, 0.5); both are
their own interpolants, so every value is exact up to rounding.  2D, u = (x^2 - y / 2, -x y + y^2) on [0, 1] x [0, 2]:
  Lap u = (2, 2), div u = x + 2 y, grad div u = (1, 2), curl u = -y + 1 / 2;  |Omega| = 2, |dOmega| = 6, int div u = 2 (1/2 + 2) = 5.
3D, u = (x^2 - y z, -2 x y + z^2, y + x z) on [0, 1] x [0, 2] x [0, 1.5]:
  Lap u = (2, 2, 0), div u = x, grad div u = (1, 0, 0), curl u = (1 - 2 z, -y - z, -2 y + z);  |Omega| = 3, |dOmega| = 13, int div u = 3 / 2.
By the divergence theorem, summed over the groups, with sigma = p I - tau and the constant f = div sigma = g - nu (Lap u + grad div u)
(symmetric form) or g - nu Lap u (gradient form):
  area = |dOmega|, flux = int div u, pressure force + viscous force = |Omega| f,
  torque = int (x - centre) x f (symmetric sigma) and int ((x - centre) x f - nu curl u) for the gradient form, whose sigma is not symmetric:
  int_dOmega eps_ijk r_j sigma_kl n_l = int eps_ijk (sigma_kj + r_j f_k), and eps_ijk (-nu d_j u_k) = -nu (curl u)_i."""
import numpy as np
import pytest

import diagnostics_reference as R
import probe_reference as PR
import surface_reference as SR
from conftest import Problem

LD = np.longdouble
G_P = (2.0, -1.0, 0.5)


def all_faces(p):
    from navierstokes_project_nm4pde_amd.problem import boundary_faces
    return boundary_faces(p.mesh)


def box_mean(fn, hi):
    """the integral of fn(X [n][dim]) over [0, hi] by the 2-point tensor Gauss rule (exact for the linear integrands used here), long double"""
    t, w = np.polynomial.legendre.leggauss(2)
    axes = [(LD(b) * (1 + t.astype(LD)) / 2, LD(b) * w.astype(LD) / 2) for b in hi]
    pts = np.stack(np.meshgrid(*[a[0] for a in axes], indexing="ij"), axis=-1).reshape(-1, len(hi))
    W = np.ones(1, dtype=LD)
    for a in axes:
        W = np.multiply.outer(W, a[1])
    return (W.reshape(-1, 1) * fn(pts)).sum(axis=0)


def closed_forms(dim, nu, form, centre):
    hi = [1.0, 2.0, 1.5][:dim]
    vol = float(np.prod(hi))
    g = np.array(G_P[:dim], dtype=LD)
    lap, gdiv = (np.array([2, 2], dtype=LD), np.array([1, 2], dtype=LD)) if dim == 2 else (np.array([2, 2, 0], dtype=LD), np.array([1, 0, 0], dtype=LD))
    f = g - LD(nu) * (lap + gdiv if form == SR.SYMMETRIC else lap)
    c = np.asarray(centre, dtype=LD)

    def moment(X):
        r = X - c
        if dim == 2:
            m = (r[:, 0] * f[1] - r[:, 1] * f[0])[:, None]
            curl = (-X[:, 1] + LD(1) / 2)[:, None]
        else:
            m = np.stack([r[:, 1] * f[2] - r[:, 2] * f[1], r[:, 2] * f[0] - r[:, 0] * f[2], r[:, 0] * f[1] - r[:, 1] * f[0]], axis=1)
            curl = np.stack([1 - 2 * X[:, 2], -X[:, 1] - X[:, 2], -2 * X[:, 1] + X[:, 2]], axis=1)
        return m if form == SR.SYMMETRIC else m - LD(nu) * curl
    return {"area": 6.0 if dim == 2 else 13.0, "flux": 5.0 if dim == 2 else 1.5, "force": (vol * f).astype(np.float64),
            "torque": box_mean(moment, hi).astype(np.float64)}


def check_closed_forms(dim, ref, tot, nu, form, centre, slack=1.0):
    """the totals `tot` summed over the groups against the closed forms, under the summed bounds of the helper `ref` (times slack)"""
    want = closed_forms(dim, nu, form, centre)
    b = {k: SR.total_bound(ref, k).sum(axis=0) * slack for k in SR.TOTALS}
    assert abs(tot["area"].sum() - want["area"]) <= b["area"]
    assert abs(tot["flux"].sum() - want["flux"]) <= b["flux"]
    force = (tot["force_pressure"] + tot["force_viscous"]).sum(axis=0)
    assert (np.abs(force[:dim] - want["force"]) <= (b["force_pressure"] + b["force_viscous"])[:dim]).all(), (force, want["force"])
    tq = tot["torque"].sum(axis=0)
    assert (np.abs(tq - want["torque"]) <= b["torque"]).all(), (tq, want["torque"])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("form", [SR.SYMMETRIC, SR.GRADIENT])
def test_quadratic_state_on_the_box_gives_the_closed_forms(dim, form):
    p = Problem("box", dim)
    cells, lfs, groups = all_faces(p)
    assert p.dofs.n_cells == {2: 18, 3: 108}[dim] and (dim == 3 or len(cells) == 12)
    assert set(lfs.tolist()) == set(range(dim + 1))                                  # every local face number occurs
    assert (np.bincount(cells) == 2).sum() >= 1                                      # some cells have two boundary faces
    nu, centre = 0.05, [0.3, 0.7, 0.2][:dim]
    state = PR.quadratic_state(p.dofs, G_P)
    ref = SR.surface(p.mesh, p.dofs, state, cells, lfs, groups, nu=nu, form=form, centre=centre)
    # G at every face node is the analytic gradient, the pressure the linear one
    _, G = R.quadratic_field(ref["x"].reshape(-1, dim).astype(LD))
    scale = np.abs(G).max()
    assert np.abs(ref["G"].reshape(-1, dim, dim) - G.astype(np.float64)).max() <= 1e-14 * scale
    assert np.abs(ref["faces"]["pressure"][:, :, 0] - (7.0 + ref["x"] @ np.array(G_P[:dim]))).max() <= 1e-14 * 10
    # the stresses from the analytic gradient and the helper's own normal
    n = ref["faces"]["normal"]
    Gf = G.astype(np.float64).reshape(ref["G"].shape)
    tau = nu * (Gf + np.swapaxes(Gf, 2, 3)) if form == SR.SYMMETRIC else nu * Gf
    tn = (tau * n[:, :, None, :]).sum(axis=3)
    t = ref["faces"]["pressure"] * n - tn
    s = -(tn - (n * tn).sum(axis=2, keepdims=True) * n)
    assert np.abs(ref["faces"]["traction"] - t).max() <= 1e-13 and np.abs(ref["faces"]["shear"] - s).max() <= 1e-13
    assert np.abs((ref["faces"]["shear"] * n).sum(axis=2)).max() <= 1e-14           # the shear is tangential
    assert np.abs(np.linalg.norm(n, axis=2) - 1).max() <= 1e-15
    # the normals of a box are the axes, outward
    mid = ref["x"][:, :dim].mean(axis=1)
    hi = np.array([1.0, 2.0, 1.5][:dim])
    axis = np.argmax(np.abs(n[:, 0]), axis=1)
    side = np.where(np.abs(mid[np.arange(len(mid)), axis]) < 1e-12, -1.0, 1.0)
    assert np.allclose(n[np.arange(len(n)), 0, axis], side, atol=1e-14)
    assert np.allclose(mid[np.arange(len(mid)), axis], np.where(side > 0, hi[axis], 0.0), atol=1e-12)
    # the recovered values at a surface node: every face of the patch gives the analytic value at the node, so the mean is that value
    # (the traction where all faces of the patch lie in one plane: a group may run round an edge of the box)
    lay = ref["layout"]
    flat = 0
    for f in range(len(cells)):
        for j, sn in enumerate(lay["face_nodes"][f]):
            assert abs(ref["nodes"]["pressure"][sn, 0] - ref["faces"]["pressure"][f, j, 0]) <= 1e-13
            if np.abs(ref["nodes"]["normal"][sn] - n[f, j]).max() <= 1e-12:
                flat += 1
                assert np.abs(ref["nodes"]["traction"][sn] - ref["faces"]["traction"][f, j]).max() <= 1e-13
                assert np.abs(ref["nodes"]["shear"][sn] - ref["faces"]["shear"][f, j]).max() <= 1e-13
    assert flat > len(cells)
    # seams: a corner node belongs to one surface node per group that holds it
    assert len(lay["nodes"]) > len(np.unique(lay["nodes"]))
    assert np.all(np.diff(lay["node_groups"] * 10 ** 6 + lay["nodes"]) > 0)          # ascending group, then ascending node
    # totals, summed over the groups, against the divergence theorem
    check_closed_forms(dim, ref, ref["totals"], nu, form, centre)
    assert ref["n_faces"].sum() == len(cells)
    assert ref["totals"]["torque"].shape == (len(ref["n_faces"]), 3 if dim == 3 else 1)


MESHES = [("box", 2, 1), ("box", 3, 1), ("cylinder", 2, 1), ("cylinder", 2, 2), ("cylinder", 3, 1)]


@pytest.mark.parametrize("kind,dim,level", MESHES)
def test_the_float64_run_is_within_the_derived_bound_of_the_long_double_run(kind, dim, level):
    p = Problem(kind, dim) if kind == "box" else Problem(kind, dim, level)
    cells, lfs, groups = all_faces(p)
    state = PR.quadratic_state(p.dofs, G_P) if kind == "box" else p.smooth_velocity()
    centre = [0.5, 0.2, 0.205][:dim] if dim == 3 else [0.2, 0.2]
    for form in (SR.SYMMETRIC, SR.GRADIENT):
        ref = SR.surface(p.mesh, p.dofs, state, cells, lfs, groups, nu=p.nu, form=form, centre=centre)
        worst = 0.0
        for k in SR.TOTALS:
            d, b = np.abs(ref["totals64"][k] - ref["totals"][k]), SR.total_bound(ref, k)
            assert (d <= b).all(), (k, d, b)
            worst = max(worst, float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1), 0))))
        print(kind, dim, level, form, "largest |float64 - long double| / bound = %.3f" % worst)
        for k in SR.FIELDS:                                                          # the fields: the standing 1e-12 X holds for the float64 run
            assert np.isfinite(ref["faces_X"][k]).all(), k                           # every entry has a finite bound: none is exempted
            assert SR.field_ratio(ref["faces64"][k], ref["faces"][k], ref["faces_X"][k]) <= 1e-12, k
        for k in SR.NODE_FIELDS:
            assert SR.field_ratio(ref["nodes64"][k], ref["nodes"][k], ref["nodes_X"][k]) <= 1e-12, k
        if kind == "cylinder":                                                       # against a vacuous pass of the GPU parity test
            ob = groups.max()
            assert ob == 3 and len(ref["n_faces"]) == 4
            on = ref["layout"]["node_groups"] == ob
            assert (np.abs(ref["nodes"]["shear"][on]).max(axis=1) > 0).mean() > 0.9
            want = 2 * np.pi * 0.05 * (0.41 if dim == 3 else 1.0)
            assert abs(ref["totals"]["area"][ob] - want) <= 0.01 * want
            if level == 1:
                assert ref["n_faces"].tolist() == ([48, 48, 744, 128] if dim == 3 else [6, 6, 36, 16])
