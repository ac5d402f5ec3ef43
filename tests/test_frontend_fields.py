"""CPU suite: nsxh_write_vtu_fields (DoFs.write_vtu_fields) writes nsxh_write_vtu's files plus the PointData arrays "vorticity" and
"q_criterion", taken at the cell vertices from node-indexed arrays."""
import re

import numpy as np
import pytest

from conftest import Problem

ARRAY = r'<DataArray type="Float64" Name="%s"[^>]*>\n(.*?)</DataArray>\n'


@pytest.mark.parametrize("dim", [2, 3])
def test_the_file_is_write_vtus_plus_two_arrays_at_the_vertices(tmp_path, dim):
    p = Problem("box", dim)
    d = p.dofs
    rng = np.random.default_rng(3)
    x = rng.standard_normal(d.n_dofs)
    n_nodes, nw = d.n_u // dim, 3 if dim == 3 else 1
    vort, q = rng.standard_normal((n_nodes, nw)), rng.standard_normal(n_nodes)
    d.write_vtu(x, tmp_path / "plain", "out", 7)
    d.write_vtu_fields(x, vort, q, tmp_path / "fields", "out", 7)
    plain = (tmp_path / "plain" / "out_7.0.vtu").read_text()
    text = (tmp_path / "fields" / "out_7.0.vtu").read_text()
    stripped = text
    for name in ("vorticity", "q_criterion"):
        assert len(re.findall(ARRAY % name, text, flags=re.S)) == 1 and name not in plain
        stripped = re.sub(ARRAY % name, "", stripped, flags=re.S)
    assert stripped == plain                                            # everything else byte for byte
    n_points = int(re.search(r'NumberOfPoints="(\d+)"', text).group(1))
    assert n_points == d.n_cells * (dim + 1)
    vertex_node = np.asarray(d.cell_dofs)[:, [(dim + 1) * v for v in range(dim + 1)]].ravel() // dim
    got_w = np.array(re.search(ARRAY % "vorticity", text, flags=re.S).group(1).split(), dtype=float).reshape(n_points, nw)
    got_q = np.array(re.search(ARRAY % "q_criterion", text, flags=re.S).group(1).split(), dtype=float)
    assert np.array_equal(got_w, vort[vertex_node]) and np.array_equal(got_q, q[vertex_node])   # 17 digits: the doubles themselves
    assert 'Name="vorticity" NumberOfComponents="%d"' % nw in text
    record = (tmp_path / "fields" / "out_7.pvtu").read_text()
    assert 'Name="vorticity"' in record and 'Name="q_criterion"' in record and "out_7.0.vtu" in record
    with pytest.raises(AssertionError):
        d.write_vtu_fields(x, vort[:, :1] if dim == 3 else np.zeros((n_nodes, 3)), q, tmp_path / "bad", "out", 0)
