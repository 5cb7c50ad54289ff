"""-m gpu: the `critical` driver through the 3-D and 2-D mains, in process: a --flows stack with a planted moving saddle
and a planted spiral sink keeps both on one track each with their classes; the .npz holds the documented arrays and the
report's rows add up to it; the filters drop rows from every array alike; the 2-D main estimates a synthetic series' flows
with the model and draws one picture per step."""
import json
import os

import numpy as np
import pytest

from test_gpu_lic_series import _png

pytestmark = pytest.mark.gpu
K, S = 3, 12
SADDLE = [np.array([3.2 + 0.45 * k, 5.3 + 0.2 * k, 6.4]) for k in range(K)]  # (x, y, z), moving
SINK = np.array([8.6, 6.4, 5.3])
ARRAYS = {"cell": np.int32, "simplex": np.uint8, "pos": np.float32, "jac": np.float64, "inv": np.float64, "cls": np.uint8,
          "vmax": np.float32, "step": np.int32, "offsets": np.int64, "track": np.int64, "frames": np.int64}


def _flows():
    """Two linear fields glued along x: a saddle (one outgoing direction) around SADDLE[k], a spiral sink around SINK."""
    A1 = np.array([[1.0, 0.2, 0.0], [0.1, -1.0, 0.0], [0.0, 0.3, -0.5]])
    A2 = np.array([[-0.5, -1.0, 0.0], [1.0, -0.5, 0.1], [0.0, 0.0, -0.7]])
    z, y, x = np.meshgrid(*[np.arange(S, dtype=np.float64)] * 3, indexing="ij")
    X = np.stack([x, y, z])
    w = 1.0 / (1.0 + np.exp(4.0 * (x - 6.0)))  # 1 on the saddle's side
    out = []
    for k in range(K):
        u1 = np.einsum("rc,c...->r...", A1, X - SADDLE[k][:, None, None, None])
        u2 = np.einsum("rc,c...->r...", A2, X - SINK[:, None, None, None])
        out.append(w * u1 + (1.0 - w) * u2)
    return (0.1 * np.stack(out)).astype(np.float32)


def _main(tmp_path, flows, extra=(), tag=""):
    from opticalflowscivis_amd import critical
    from opticalflowscivis_amd.flow3d.model.RIFE import Model
    fl, out, rep = (str(tmp_path / (tag + n)) for n in ("flows.npy", "cp.npz", "r.json"))
    np.save(fl, flows)
    doc = critical.main_rife(Model, 3, ["--flows", fl, "--chunk", "2", "--link-radius", "1.5", "--out", out, "--json", rep] +
                             list(extra))
    assert json.load(open(rep)) == json.loads(json.dumps(doc))
    return doc, dict(np.load(out))


def _adds_up(doc, z, nd):
    from opticalflowscivis_amd import ops
    N = len(z["cell"])
    assert sorted(z) == sorted(ARRAYS)
    for name, dt in ARRAYS.items():
        assert z[name].dtype == dt, name
    assert z["pos"].shape == (N, nd) and z["jac"].shape == (N, nd * nd) and z["inv"].shape == (N, 4)
    for name in ("simplex", "cls", "vmax", "step", "track"):
        assert z[name].shape == (N,), name
    assert len(doc["steps"]) == len(z["offsets"]) - 1 and z["offsets"][0] == 0 and z["offsets"][-1] == N
    assert z["frames"].tolist() == doc["frames"]
    names = np.array(ops.critical_class_names(z["cls"], nd), dtype=object)
    for j, row in enumerate(doc["steps"]):
        a, b = z["offsets"][j:j + 2]
        assert row["n_points"] == b - a == sum(row["classes"].values()) and (z["step"][a:b] == j).all()
        assert row["n_found"] >= row["n_points"]
        for n, c in row["classes"].items():
            assert c == (names[a:b] == n).sum(), n
        assert row["index_sum"] == int(np.sign(z["inv"][a:b, 2 if nd == 3 else 1]).sum())
        prev = set(z["track"][z["offsets"][j - 1]:a].tolist()) if j else set()
        assert row["births"] == sum(t not in prev for t in z["track"][a:b].tolist())
    assert sum(r["births"] for r in doc["steps"]) == doc["n_tracks"] == len(set(z["track"].tolist()))
    assert sum(r["deaths"] for r in doc["steps"][:-1]) + doc["steps"][-1]["n_points"] == doc["n_tracks"]


def test_flow3d_main_tracks_the_planted_points(tmp_path):
    from opticalflowscivis_amd import ops
    doc, z = _main(tmp_path, _flows())
    assert doc["shape"] == [S, S, S] and doc["chunk"] == 2 and doc["link_radius"] == 1.5 and doc["model"] is None
    assert doc["time_kernel_s"] > 0
    _adds_up(doc, z, 3)
    tracks = {"saddle1": set(), "spiral_sink": set()}
    for k in range(K):
        a, b = z["offsets"][k:k + 2]
        for want, p in (("saddle1", SADDLE[k]), ("spiral_sink", SINK)):
            d = np.abs(z["pos"][a:b].astype(np.float64) - p).max(1)
            i = a + int(d.argmin())
            assert d.min() < 0.02, (k, want, d.min())  # (the other field's share there is exp(-4 * 2.5))
            assert ops.critical_class_names(z["cls"][i:i + 1], 3) == [want]
            tracks[want].add(int(z["track"][i]))
    assert len(tracks["saddle1"]) == 1 and len(tracks["spiral_sink"]) == 1 and tracks["saddle1"] != tracks["spiral_sink"]


def test_filters_drop_rows_from_every_array(tmp_path):
    rng = np.random.default_rng(12)
    flows = rng.standard_normal((K, 3, 6, 7, 8)).astype(np.float32)
    _, full = _main(tmp_path, flows)
    jn = np.sqrt((full["jac"] ** 2).sum(1))
    cut = float(np.median(jn))
    doc, z = _main(tmp_path, flows, ["--classes", "saddle1,spiral_saddle2", "--min-jnorm", repr(cut)], tag="f_")
    _adds_up(doc, z, 3)
    from opticalflowscivis_amd import ops
    names = np.array(ops.critical_class_names(full["cls"], 3), dtype=object)
    keep = (jn >= cut) & ((names == "saddle1") | (names == "spiral_saddle2"))
    assert 0 < keep.sum() < len(keep)
    for name in ("cell", "simplex", "pos", "jac", "inv", "cls", "vmax", "step"):
        assert np.array_equal(z[name], full[name][keep]), name
    assert [r["n_found"] for r in doc["steps"]] == np.diff(full["offsets"]).tolist()


def test_flow2d_main_with_the_model_and_pictures(tmp_path):
    from opticalflowscivis_amd import critical
    from opticalflowscivis_amd.flow2d.model.RIFE import Model
    out, rep, shots = (str(tmp_path / n) for n in ("cp.npz", "r.json", "shots"))
    doc = critical.main_rife(Model, 2, ["--dataset", "rectangle2d", "--frames", "5", "--model",
                                        str(tmp_path / "none"), "--out", out, "--json", rep, "--png-dir", shots])
    assert json.load(open(rep)) == json.loads(json.dumps(doc))
    n = len(doc["steps"])
    assert n >= 1 and doc["shape"] == [128, 128] and len(doc["frames"]) == n + 1
    _adds_up(doc, dict(np.load(out)), 2)
    names = sorted(os.listdir(shots))
    assert names == ["critical_%03d_to_%03d.png" % (r["t_from"], r["t_to"]) for r in doc["steps"]]
    assert doc["pngs"] == [os.path.join(shots, f) for f in names]
    for f in names:
        w, h, colour, rows = _png(os.path.join(shots, f))
        assert (w, h, colour) == (128, 128, 2) and rows.shape == (128, 3 * 128)


def test_markers_are_drawn_where_the_points_are():
    from opticalflowscivis_amd import critical
    tab = {"pos": np.array([[4.2, 2.0], [0.0, 5.6]], np.float32), "cls": np.array([1, 4], np.uint8)}
    img = critical.draw_points(np.zeros((8, 9), np.float32), tab, (2.0, 1.0))  # spacing (y, x)
    assert img.shape == (8, 9, 3) and img.dtype == np.uint8
    assert img[1, 4].tolist() == [40, 220, 60] and img[1, 5].tolist() == [40, 220, 60] and img[2, 4].tolist() == [40, 220, 60]
    assert img[3, 0].tolist() == [147, 172, 255] and img[3, 1].any() and not img[6, 6].any()
    assert (img.reshape(-1, 3).any(1)).sum() == 5 + 4  # a plus, and one cut by the border
