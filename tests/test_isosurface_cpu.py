"""CPU: the numpy restatement of the isosurface definition (tests/isosurface_ref.py) against invariants it does not
assume -- closedness, orientation, the Euler characteristic, analytic area and volume -- plus the kernel's table against
the geometry, the PLY writer, mesh_stats, and the C-ABI's argument errors."""
import ctypes
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

import isosurface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _closed(mesh, euler):
    V = mesh["vertices"].shape[0]
    t = R.topology(mesh["faces"], V)
    assert t["bad_edges"] == 0 and t["degenerate"] == 0, t  # every edge in exactly two faces, in opposite directions
    assert t["used_vertices"] == V  # no vertex without a face
    assert V - t["edges"] + mesh["faces"].shape[0] == euler, t
    assert 2 * t["edges"] == 3 * mesh["faces"].shape[0]


def _inside_the_volume(mesh, shape):
    v = mesh["vertices"]
    assert v.min() > 0 and (v.max(0) < np.array(shape[::-1]) - 1).all()


def test_sphere_is_closed_and_oriented():
    f, _ = R.sphere_field(16)
    m = R.extract(f, 0.0)
    _inside_the_volume(m, f.shape)
    _closed(m, 2)
    # unit normals that point away from the centre (towards lower values)
    n = m["normals64"]
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12
    radial = m["vertices"].astype(np.float64) - np.array([7.4, 7.6, 7.2])
    assert ((n * radial).sum(1) > 0).all()
    # the geometric normal of every face agrees with its vertices' normals
    v = m["vertices"].astype(np.float64)
    fc = m["faces"]
    g = np.cross(v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]])
    assert ((g * n[fc].sum(1)).sum(1) >= 0).all()


def test_torus_has_genus_one():
    f = R.torus_field()
    m = R.extract(f, 0.0)
    _inside_the_volume(m, f.shape)
    _closed(m, 0)


def test_two_balls_are_two_spheres():
    f = R.two_balls_field()
    m = R.extract(f, 0.0)
    _inside_the_volume(m, f.shape)
    _closed(m, 4)


def test_integer_field_with_exact_hits_is_closed():
    f = R.integer_field()
    assert int((f == 0).sum()) == 30
    m = R.extract(f, 0.0)
    _closed(m, 2)
    assert (m["t"] == 0).any() or (m["t"] == 1).any()  # vertices that sit on nodes


def test_vertex_and_face_order():
    m = R.extract(R.sphere_field(16)[0], 0.0)
    key = m["owner"] * 7 + m["edge"]
    assert (np.diff(key) > 0).all()
    assert (np.diff(m["face_cell"]) >= 0).all()
    assert m["faces"].dtype == np.int32 and m["vertices"].dtype == np.float32


def test_sphere_area_and_volume_converge():
    err_a, err_v = [], []
    for n in (16, 32, 64):
        f, r = R.sphere_field(n, n / 16.0)
        m = R.extract(f, 0.0)
        a, v = R.area_volume(m["vertices"], m["faces"])
        assert v > 0
        err_a.append(abs(a / (4 * np.pi * r * r) - 1))
        err_v.append(abs(v / (4.0 / 3.0 * np.pi * r ** 3) - 1))
    assert err_a[0] > err_a[1] > err_a[2], err_a
    assert err_v[0] > err_v[1] > err_v[2], err_v


def test_spacing_scales_positions_and_rotates_normals():
    f, _ = R.sphere_field(16)
    a = R.extract(f, 0.0)
    b = R.extract(f, 0.0, spacing=(0.5, 1.0, 2.0))
    assert np.array_equal(a["faces"], b["faces"])
    assert np.array_equal(a["vertices"] * np.array([0.5, 1.0, 2.0], np.float32), b["vertices"])
    area_a, vol_a = R.area_volume(a["vertices"], a["faces"])
    area_b, vol_b = R.area_volume(b["vertices"], b["faces"])
    assert abs(vol_b / vol_a - 1.0) < 1e-6  # 0.5 * 1 * 2


def test_nonfinite_nodes_cut_holes_not_garbage():
    rng = np.random.default_rng(5)
    f = rng.standard_normal((6, 7, 8)).astype(np.float32)
    f[2, 3, 4] = np.nan
    f[4, 1, 6] = np.inf
    f[0, 0, 0] = -np.inf
    m = R.extract(f, 0.1)
    bad = ~np.isfinite(f)
    cz, cy, cx = np.unravel_index(m["face_cell"], f.shape)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                assert not bad[cz + dz, cy + dy, cx + dx].any()
    assert np.isfinite(m["vertices"]).all()


def _load_generator():
    spec = importlib.util.spec_from_file_location("gen_iso_tables", os.path.join(ROOT, "scripts", "gen_iso_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_kernel_table_is_the_generated_one_and_matches_the_geometry():
    gen = _load_generator()
    with open(os.path.join(ROOT, "opticalflowscivis_amd", "csrc", "iso_tables.hpp")) as fh:
        assert fh.read() == gen.render()
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    for ti, perm in enumerate(R.PERMS):
        for cs in range(16):
            w = gen.word(perm, cs)
            tris = [[pairs[w >> (2 + 9 * j + 3 * i) & 7] for i in range(3)] for j in range(w & 3)]
            assert tris == [[tuple(e) for e in t] for t in R.tet_triangles(perm, [(cs >> i) & 1 for i in range(4)])], (ti, cs)


def _read_ply(path):
    with open(path, "rb") as fh:
        blob = fh.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = [int(l.split()[2]) for l in lines if l.startswith("element vertex")][0]
    nf = [int(l.split()[2]) for l in lines if l.startswith("element face")][0]
    props = [l.split()[2] for l in lines if l.startswith("property float")]
    rows = np.array(struct.unpack_from("<%df" % (nv * len(props)), body, 0), np.float32).reshape(nv, len(props))
    off = 4 * nv * len(props)
    faces = np.zeros((nf, 3), np.int32)
    for i in range(nf):
        n, a, b, c = struct.unpack_from("<Biii", body, off + 13 * i)
        assert n == 3
        faces[i] = (a, b, c)
    assert off + 13 * nf == len(body)
    return props, rows, faces


def test_ply_round_trip(tmp_path):
    from opticalflowscivis_amd import isosurface
    f, _ = R.sphere_field(16)
    m = R.extract(f, 0.0, values=np.stack([f * 2, f + 1]))
    path = str(tmp_path / "m.ply")
    isosurface.write_ply(path, m["vertices"], m["normals32"], m["faces"], m["values32"])
    props, rows, faces = _read_ply(path)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "value0", "value1"]
    assert np.array_equal(rows[:, :3], m["vertices"]) and np.array_equal(rows[:, 3:6], m["normals32"])
    assert np.array_equal(rows[:, 6:], m["values32"]) and np.array_equal(faces, m["faces"])
    isosurface.write_ply(path, m["vertices"][:0], m["normals32"][:0], m["faces"][:0])
    props, rows, faces = _read_ply(path)
    assert rows.shape == (0, 6) and faces.shape == (0, 3)


def test_mesh_stats_matches_numpy():
    from opticalflowscivis_amd import isosurface
    f, r = R.sphere_field(16)
    m = R.extract(f, 0.0)
    st = isosurface.mesh_stats(m["vertices"], m["faces"])
    a, v = R.area_volume(m["vertices"], m["faces"])
    assert abs(st["area"] - a) < 1e-9 * a and abs(st["volume"] - v) < 1e-9 * v and st["boundary_edges"] == 0
    assert np.allclose(st["bbox"], [m["vertices"].min(0), m["vertices"].max(0)])
    open_ = isosurface.mesh_stats(m["vertices"], m["faces"][1:])
    assert open_["boundary_edges"] == 3
    assert isosurface.mesh_stats(m["vertices"][:0], m["faces"][:0]) == {"area": 0.0, "volume": 0.0, "bbox": None,
                                                                        "boundary_edges": 0}


def test_c_abi_errors_without_gpu():
    """Every argument error is returned before anything is launched, so it is testable on the CPU."""
    from opticalflowscivis_amd import _lib
    lib = _lib.lib()
    h = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    P = 8 * 8 * 8
    assert lib.fs_iso3d_ws_bytes(2, 8, 8, 8) == 2 * 2 * 64 * 4 + 2 * P
    assert lib.fs_iso3d_ws_bytes(1, 1, 8, 8) == -2 and lib.fs_iso3d_ws_bytes(0, 8, 8, 8) == -2
    assert lib.fs_iso3d_ws_bytes(1, 2048, 2048, 2048) == -2  # more than 2^31 - 1 nodes
    assert lib.fs_iso3d_ws_bytes(70000, 1024, 1024, 2) == -2  # more than 2^31 - 1 rows
    # count
    assert lib.fs_iso_count3d(None, 1, 8, 8, 8, P, 0.5, 16, None) == 1
    assert lib.fs_iso_count3d(16, 1, 8, 8, 8, P, 0.5, None, None) == 1
    assert lib.fs_iso_count3d(16, 1, 8, 1, 8, P, 0.5, 16, None) == 2      # an extent below 2
    assert lib.fs_iso_count3d(16, 2, 8, 8, 8, P - 1, 0.5, 16, None) == 2  # sstride too small
    assert lib.fs_iso_count3d(16, 0, 8, 8, 8, P, 0.5, 16, None) == 2      # K
    assert lib.fs_iso_count3d(16, 1, 8, 8, 8, P, float("nan"), 16, None) == 3
    assert lib.fs_iso_count3d(16, 1, 8, 8, 8, P, float("inf"), 16, None) == 3
    assert lib.fs_iso_count3d(16, 1, 8, 8, 8, P, 1e300, 16, None) == 3    # not finite as fp32
    # emit: volumes, K, D, H, W, sstride, iso, spacing, ws, row_offsets, V, T, values, F, vertices, normals, values_out,
    # faces, status, stream
    ok = [16, 1, 8, 8, 8, P, 0.5, h, 16, 16, 10, 10, 16, 2, 16, 16, 16, 16, 16, None]

    def emit(**kw):
        names = ("volumes", "K", "D", "H", "W", "sstride", "iso", "spacing", "ws", "row_offsets", "V", "T", "values", "F",
                 "vertices", "normals", "values_out", "faces", "status", "stream")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.fs_iso_emit3d(*a)

    for name in ("volumes", "spacing", "ws", "row_offsets", "status", "vertices", "faces", "values", "values_out"):
        assert emit(**{name: None}) == 1, name
    assert emit(W=1) == 2 and emit(sstride=P - 1) == 2 and emit(K=0) == 2 and emit(F=9) == 2 and emit(F=-1) == 2
    assert emit(iso=float("nan")) == 3 and emit(V=-1) == 3 and emit(T=-1) == 3 and emit(ws=18) == 3
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        assert emit(spacing=(ctypes.c_double * 3)(1.0, bad, 1.0)) == 3, bad
    # nothing to write: FS_OK with nothing launched (normals and values may be absent)
    assert emit(V=0, T=0, vertices=None, faces=None, normals=None, values=None, values_out=None, F=0) == 0


def test_ops_isosurface_refuses_cpu_tensors_and_bad_arguments():
    from opticalflowscivis_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.isosurface(torch.rand(1, 8, 8, 8), 0.5)
    with pytest.raises(ValueError):
        ops.isosurface_cost((8, 8, 1))
    assert ops.isosurface_cost((8, 8, 8), 2, op="count") == (2 * (5 * 512 + 8 * 64), 0)
    assert ops.isosurface_cost((8, 8, 8), 1, V=10, T=20, F=2, op="emit") == (512 + 10 * 32 + 240, 0)
