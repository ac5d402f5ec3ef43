"""GPU suite: the host mirror's opt-in lattice image.  navier_stokes2D level:1 3 4 with NSX_LATTICE=64,16 writes one VTK ImageData file per
output step beside the VTU; the last one holds what Nsx.get_lattice() gives behind the same three steps driven from Python (the recipe of
tests/test_gpu_executables.py and tests/test_gpu_probes.py) -- the point count, the lattice, the mask exactly and the velocity and pressure
under the standing tolerance 1e-12 S of tests/test_gpu_lattice.py.  The file is ASCII: it is compared after parsing, not byte by byte.
Without NSX_LATTICE nothing changes: no .vti, the same console output."""
import os
import re
import subprocess

import numpy as np
import pytest

import lattice_reference as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def read_vti(path):
    """{"extent", "origin", "spacing", arrays by name [n_points][n_components]} of an ASCII ImageData file"""
    text = open(path).read()
    head = re.search(r'<ImageData WholeExtent="([^"]*)" Origin="([^"]*)" Spacing="([^"]*)">', text)
    out = {"extent": [int(x) for x in head.group(1).split()], "origin": [float(x) for x in head.group(2).split()],
           "spacing": [float(x) for x in head.group(3).split()]}
    for m in re.finditer(r'<DataArray type="(\w+)" Name="(\w+)"(?: NumberOfComponents="(\d+)")? format="ascii">\n(.*?)</DataArray>', text, flags=re.S):
        kind, name, nc, body = m.groups()
        out[name] = np.array(body.split(), dtype=np.int32 if kind == "Int32" else np.float64).reshape(-1, int(nc or 1))
    return out


def test_executable_writes_the_lattice_image_only_when_asked(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    from navierstokes_project_nm4pde_amd import nsx
    from navierstokes_project_nm4pde_amd.frontend import DoFs, Mesh, Tables
    from navierstokes_project_nm4pde_amd.problem import InletVelocity, cylinder_boundary_values
    dim, counts = 2, (64, 16)
    exe = os.path.join(ROOT, "navierstokes_project_nm4pde_amd", "host", "navier_stokes%dD" % dim)
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    env = {k: v for k, v in os.environ.items() if k not in ("NSX_LATTICE", "NSX_FIELDS")}
    out = subprocess.run([exe, "level:1", "3", "4"], cwd=with_dir, env=dict(env, NSX_LATTICE="64,16"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain = subprocess.run([exe, "level:1", "3", "4"], cwd=without_dir, env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr

    def untimed(text):
        return [line for line in text.splitlines() if not re.search(r"[Tt]ime taken|seconds|elapsed", line)]
    assert untimed(out.stdout) == untimed(plain.stdout) and len(untimed(out.stdout)) > 10
    assert not [f for f in os.listdir(without_dir / "output2D_1") if f.endswith(".vti")]
    files = sorted(f for f in os.listdir(with_dir / "output2D_1") if f.endswith(".vti"))
    assert files == ["lattice-navier-stokes-2D_%d.vti" % k for k in range(4)]           # output(0) and the three steps
    bad = subprocess.run([exe, "level:1", "1", "4"], cwd=without_dir, env=dict(env, NSX_LATTICE="64"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "NSX_LATTICE" in bad.stdout + bad.stderr
    img = read_vti(with_dir / "output2D_1" / files[-1])
    first = read_vti(with_dir / "output2D_1" / files[0])
    assert not first["velocity"].any() and not first["pressure"].any()                  # the initial condition is zero
    # the same three steps from Python
    mesh = Mesh.cylinder(dim, 1).partition(1, 4)
    dofs, tables = DoFs(mesh, "colour"), Tables(dim)
    dt = 0.01
    origin, spacing = LR.span(mesh, counts)
    dev = nsx.Nsx(dofs, tables, 1e-3, dt)
    try:
        dev.set_solution(np.zeros(dofs.n_dofs))
        n_found = dev.set_lattice(origin, spacing, counts)
        inlet = InletVelocity(dim, 2)
        t = 0.0
        for step in range(3):
            t += dt
            if step == 0:
                dev.assemble(nsx.TEMAM)
            else:
                dev.assemble_time_step(nsx.TEMAM)
            dev.apply_boundary_values(*cylinder_boundary_values(dofs, inlet, t))
            dev.solve_time_step(3, inner_maxiter=10000)
        dev.eval_lattice(nsx.LATTICE_VELOCITY | nsx.LATTICE_PRESSURE)
        vel = dev.get_lattice(nsx.LATTICE_VELOCITY).reshape(dim, -1).T
        pres = dev.get_lattice(nsx.LATTICE_PRESSURE).reshape(-1)
        cells = dev.lattice_cells().ravel()
        ref = LR.evaluate(mesh, dofs, dev.solution, origin, spacing, counts)
    finally:
        dev.close()
    assert img["extent"] == [0, 63, 0, 15, 0, 0] and len(img["cell_id"]) == 64 * 16
    assert img["origin"] == [origin[0], origin[1], 0.0] and img["spacing"] == [spacing[0], spacing[1], 1.0]   # 17 digits: the same doubles
    assert np.array_equal(img["cell_id"][:, 0], cells) and 0 < n_found == (cells >= 0).sum() < len(cells)
    assert img["velocity"].shape == (1024, 3) and not img["velocity"][:, 2].any() and "vorticity" not in img
    du = np.abs(img["velocity"][:, :2] - vel)
    dp = np.abs(img["pressure"][:, 0] - pres)
    print("vti against get_lattice: velocity %.2e, pressure %.2e (absolute)" % (du.max(), dp.max()))
    assert (du <= TOL * ref["S_u"]).all() and (dp <= TOL * ref["S_p"]).all()
    assert np.abs(vel).max() > 0.01 and not img["velocity"][cells < 0].any() and not img["pressure"][cells < 0].any()
