"""-m gpu: the flow3d `isosurface` entry point.  main3d on a 3-frame 12^3 --seq (PLY files, chunked) and on a
[K, NP, *sp] --field with --plane and --color-field (npz files): the files read back equal to ops.isosurface called here,
and the report's area, volume and boundary_edges match numpy on those arrays."""
import json
import os

import numpy as np
import pytest
import torch

import isosurface_ref as R
from test_isosurface_cpu import _read_ply

pytestmark = pytest.mark.gpu


def _series(K=3, S=12):
    """[K, S, S, S] fp32: a ball that drifts along x, empty space around it."""
    z, y, x = np.indices((S, S, S)).astype(np.float32)
    return np.stack([1.0 - np.sqrt((x - 4.3 - 0.7 * k) ** 2 + (y - 5.6) ** 2 + (z - 5.2) ** 2) / 4.0 for k in range(K)]).astype(np.float32)


def _op(vols, iso, spacing=1.0, values=None):
    from opticalflowscivis_amd import ops
    w = None if values is None else torch.from_numpy(values).cuda()
    r = ops.isosurface(torch.from_numpy(vols).cuda(), iso, spacing, True, w)
    ops.isosurface_check(r)
    return {k: t.cpu().numpy() for k, t in r.items()}


def _check_report(doc, r, K, dt):
    assert [f["frame"] for f in doc["frames"]] == list(range(K))
    assert [f["time"] for f in doc["frames"]] == [j * dt for j in range(K)]
    for k, row in enumerate(doc["frames"]):
        v = r["vertices"][r["vertex_offsets"][k]:r["vertex_offsets"][k + 1]]
        f = r["faces"][r["face_offsets"][k]:r["face_offsets"][k + 1]]
        area, vol = R.area_volume(v, f)
        t = R.topology(f, len(v))
        assert row["vertices"] == len(v) and row["faces"] == len(f) and row["status"] == 0
        assert row["area"] == pytest.approx(area, rel=1e-9) and row["volume"] == pytest.approx(vol, rel=1e-9)
        assert row["boundary_edges"] == t["bad_edges"] == 0 and vol > 0
        assert np.allclose(row["bbox"], [v.min(0), v.max(0)])


def test_flow3d_isosurface_of_a_series_to_ply(tmp_path):
    from opticalflowscivis_amd import isosurface
    from opticalflowscivis_amd.flow3d import isosurface as entry  # noqa: F401  (the module imports)
    K = 3
    frames = _series(K)
    seq, js, meshes = (str(tmp_path / n) for n in ("frames.npy", "r.json", "meshes"))
    np.save(seq, frames)
    doc = isosurface.main3d(["--seq", seq, "--iso", "0.5", "--mesh-dir", meshes, "--format", "ply", "--chunk", "2",
                             "--dt", "0.5", "--json", js])
    assert json.load(open(js)) == json.loads(json.dumps(doc))
    r = _op(frames, 0.5)
    assert sorted(os.listdir(meshes)) == ["frame_%04d.ply" % j for j in range(K)]
    for k in range(K):
        props, rows, faces = _read_ply(os.path.join(meshes, "frame_%04d.ply" % k))
        v0, v1 = r["vertex_offsets"][k:k + 2]
        f0, f1 = r["face_offsets"][k:k + 2]
        assert props == ["x", "y", "z", "nx", "ny", "nz"]
        np.testing.assert_array_equal(rows[:, :3].view(np.uint32), r["vertices"][v0:v1].view(np.uint32))
        np.testing.assert_array_equal(rows[:, 3:].view(np.uint32), r["normals"][v0:v1].view(np.uint32))
        np.testing.assert_array_equal(faces, r["faces"][f0:f1])
    _check_report(doc, r, K, 0.5)
    assert doc["frames"][0]["vertices"] > 100


def test_flow3d_isosurface_of_a_field_plane_with_colours_to_npz(tmp_path):
    from opticalflowscivis_amd import isosurface
    K = 2
    s = _series(K)
    field = np.stack([2.0 - 3.0 * s, s, s * s], 1)  # [K, NP = 3, 12, 12, 12]
    fld, js, meshes = (str(tmp_path / n) for n in ("vg.npy", "r.json", "meshes"))
    np.save(fld, field)
    doc = isosurface.main3d(["--field", fld, "--plane", "1", "--iso", "0.4", "--color-field", fld, "--color-plane", "2",
                             "--spacing", "0.5", "1", "2", "--mesh-dir", meshes, "--format", "npz", "--json", js])
    assert doc["plane"] == 1 and doc["color_plane"] == 2 and doc["shape"] == [12, 12, 12]
    r = _op(np.ascontiguousarray(field[:, 1]), 0.4, (0.5, 1.0, 2.0), np.ascontiguousarray(field[:, 2:3]))
    for k in range(K):
        z = np.load(os.path.join(meshes, "frame_%04d.npz" % k))
        v0, v1 = r["vertex_offsets"][k:k + 2]
        f0, f1 = r["face_offsets"][k:k + 2]
        for name in ("vertices", "normals", "values"):
            np.testing.assert_array_equal(z[name].view(np.uint32), r[name][v0:v1].view(np.uint32))
        np.testing.assert_array_equal(z["faces"], r["faces"][f0:f1])
        assert z["values"].shape == (v1 - v0, 1) and z["faces"].dtype == np.int32
    _check_report(doc, r, K, 1.0)
