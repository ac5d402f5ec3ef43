"""CPU suite: the four VTK text writers of the host library (nsxh_write_vtu, nsxh_write_vtu_fields, nsxh_write_vtu_stats, nsxh_write_vti) write
the same bytes as before they shared one writer.  The fields are small dyadic rationals, so that 17 significant digits print them in one
way only, and every file is compared through its SHA-256.

The digests below were recorded from a build of the PARENT of the commit that introduced the shared writer (three separate copies of the
file prologue), not from the shared writer itself."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from conftest import Problem

DIGESTS = {
    2: {
        "out_7.0.vtu": "2ee57b710c5d3cc042ac321a57d0223f7723ae7c77a5b254ffd3d56f049ec746",
        "out_7.pvtu": "ef2b6deef1f0f72f8fb38e70112fb70b4833468c119e66417d895a0d0b1a38b7",
        "fields_7.0.vtu": "34e7b7cd0ede2ee9b7b2dedf32dc4eca40c2ff7ef19c6ca12a4c799839a56857",
        "fields_7.pvtu": "7b8440f360515aae70e54a0e400596002db196e5a15d53ebc9147c1a7e802add",
        "stats.vtu": "8483f35743bb099feb37c17741b39ed0845e92cb9e14aedfa81c9ab59f9048cb",
        "lattice_3.vti": "24fef8915cb3efc8ca8fd6bb892bedd0aeb9fc5c04ed72a2554debcb400c7fed",
        "lattice_plain_3.vti": "fe3fc9717b339befff2e58523e4762182c9886aa0b65f40db942bb15f2b1d07a",
    },
    3: {
        "out_7.0.vtu": "7142c3d33aad1c24ddc343c20f1e3ba726701fd134aa9794db371d5eedad69c1",
        "out_7.pvtu": "ef2b6deef1f0f72f8fb38e70112fb70b4833468c119e66417d895a0d0b1a38b7",
        "fields_7.0.vtu": "5ca1fd6cdc3c04d056da70c75cdece02ea3ce0cd4109515120dcc5e85b775fb8",
        "fields_7.pvtu": "d49c63945029211ce75602051542ec9ca8f50ae8fa7f2e79160931357c6dbb5a",
        "stats.vtu": "6c0d7c92276640df7b8fc1b48cef69f4f815cbc392ecbc4a3048b7d2c47ed695",
        "lattice_3.vti": "34869b6c12bd1d80a2c3ddf9519513e54693392b8daa4d66fec921c6b9205ef2",
        "lattice_plain_3.vti": "b49982a11c4d86ae790c5616abd5ebdaa1f5aba7e377f21b2b2d8075c69d74b5",
    },
}


def dyadic(rng, *shape):
    return rng.integers(-512, 513, size=shape).astype(np.float64) / 64.0


def write_all(d, dim, out):
    """every writer once into the directory `out` (made by the writers, two levels deep); {file name: SHA-256}"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ptr = lambda a: a.ctypes.data_as(ip if a.dtype == np.int32 else dp)
    rng = np.random.default_rng(11)
    n_nodes, nw, nsym = d.n_u // dim, 3 if dim == 3 else 1, dim * (dim + 1) // 2
    x = dyadic(rng, d.n_dofs)
    vort, q = dyadic(rng, n_nodes, nw), dyadic(rng, n_nodes)
    d.write_vtu(x, out, "out", 7)
    d.write_vtu_fields(x, vort, q, out, "fields", 7)
    lib = d._lib
    mean_u, mean_p, rms_u = dyadic(rng, n_nodes, dim), dyadic(rng, d.n_p), dyadic(rng, n_nodes, dim)
    stress, tke = dyadic(rng, n_nodes, nsym), dyadic(rng, n_nodes)
    lib.nsxh_write_vtu_stats.restype = C.c_int
    lib.nsxh_write_vtu_stats.argtypes = [C.c_void_p] + [dp] * 5 + [C.c_char_p] * 2
    assert lib.nsxh_write_vtu_stats(d._h, ptr(mean_u), ptr(mean_p), ptr(rms_u), ptr(stress), ptr(tke), str(out).encode(), b"stats") == 0
    counts = np.array([5, 4] if dim == 2 else [4, 3, 3], dtype=np.int32)
    n = int(np.prod(counts))
    origin, spacing = dyadic(rng, dim), np.array([0.25, 0.5, 0.125][:dim])
    vel, pre, lvort = dyadic(rng, dim, n), dyadic(rng, n), dyadic(rng, nw, n)
    cells = rng.integers(-1, d.n_cells, size=n).astype(np.int32)
    lib.nsxh_write_vti.restype = C.c_int
    lib.nsxh_write_vti.argtypes = [C.c_int, dp, dp, ip, dp, dp, ip, dp, C.c_int, C.c_char_p, C.c_char_p, C.c_uint]
    assert lib.nsxh_write_vti(dim, ptr(origin), ptr(spacing), ptr(counts), ptr(vel), ptr(pre), ptr(cells), ptr(lvort), nw, str(out).encode(), b"lattice", 3) == 0
    assert lib.nsxh_write_vti(dim, ptr(origin), ptr(spacing), ptr(counts), ptr(vel), ptr(pre), ptr(cells), None, 0, str(out).encode(), b"lattice_plain", 3) == 0
    return {f.name: hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(out.iterdir())}


@pytest.mark.parametrize("dim,n_cells", [(2, 18), (3, 108)])
def test_every_writer_writes_the_bytes_of_the_parent_commit(tmp_path, dim, n_cells):
    d = Problem("box", dim).dofs
    assert d.n_cells == n_cells
    got = write_all(d, dim, tmp_path / "a" / "b")
    assert sorted(got) == sorted(DIGESTS[dim])
    for name, digest in DIGESTS[dim].items():
        print(name, got[name])
        assert got[name] == digest, name


def test_null_arguments_and_unwritable_paths_are_refused(tmp_path):
    d = Problem("box", 2).dofs
    lib, dp = d._lib, C.POINTER(C.c_double)
    x = np.zeros(d.n_dofs)
    xp = x.ctypes.data_as(dp)
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    bad = str(blocker / "sub").encode()
    assert lib.nsxh_write_vtu(d._h, None, str(tmp_path).encode(), b"out", 0) == -1
    assert lib.nsxh_write_vtu(d._h, xp, None, b"out", 0) == -1
    assert lib.nsxh_write_vtu(d._h, xp, bad, b"out", 0) == -1
    assert lib.nsxh_write_vtu_fields(d._h, xp, xp, 2, xp, str(tmp_path).encode(), b"out", 0) == -1    # 2 vorticity components: neither 2D nor 3D
    assert lib.nsxh_write_vtu_fields(d._h, xp, xp, 1, xp, bad, b"out", 0) == -1
    lib.nsxh_write_vtu_stats.restype = C.c_int
    lib.nsxh_write_vtu_stats.argtypes = [C.c_void_p] + [dp] * 5 + [C.c_char_p] * 2
    assert lib.nsxh_write_vtu_stats(d._h, xp, xp, xp, xp, None, str(tmp_path).encode(), b"stats") == -1
    assert lib.nsxh_write_vtu_stats(d._h, xp, xp, xp, xp, xp, bad, b"stats") == -1
    assert sorted(f.name for f in tmp_path.iterdir()) == ["file"]
