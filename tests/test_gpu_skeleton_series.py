"""-m gpu: the `skeleton` driver through the 2-D and 3-D mains, in process, on a written --flows stack of three double
wells (tests/streamline_fields.py): every step has one saddle whose two unstable lines end in the two sinks; the .npz
holds the documented arrays and they add up; the pictures (2-D) and the VTK line files (3-D) are written and read back."""
import json
import os

import numpy as np
import pytest

import streamline_fields as fields
from test_gpu_lic_series import _png

pytestmark = pytest.mark.gpu
K = 3
LINE_ARRAYS = {"line_offsets": np.int64, "line_verts": np.float32, "line_step": np.int32, "line_origin": np.int64,
               "line_manifold": np.uint8, "line_dim": np.uint8, "line_end": np.uint8, "line_target": np.int64}
CAPTURED, OUT = 4, 1


def _main(tmp_path, nd, extra=()):
    from opticalflowscivis_amd import skeleton
    Model = __import__("opticalflowscivis_amd.flow%dd.model.RIFE" % nd, fromlist=["Model"]).Model
    f, c, s = fields.double_well(nd)
    fl, out, rep = (str(tmp_path / n) for n in ("flows.npy", "skel.npz", "r.json"))
    np.save(fl, np.stack([f * (1.0 + 0.5 * k) for k in range(K)]))  # (the same lines at every step: the field is normalised)
    doc = skeleton.main_rife(Model, nd, ["--flows", fl, "--chunk", "2", "--max-steps", "400", "--out", out, "--json", rep] +
                             list(extra))
    assert json.load(open(rep)) == json.loads(json.dumps(doc))
    return doc, dict(np.load(out)), c, s


def _adds_up(doc, z, nd, lines_per_step):
    from opticalflowscivis_amd import ops
    for name, dt in LINE_ARRAYS.items():
        assert z[name].dtype == dt, name
    L = len(z["line_step"])
    off = z["line_offsets"]
    V = len(z["line_verts"])
    assert L == K * lines_per_step and off.shape == (L + 1,) and off[0] == 0 and off[-1] == V
    assert (np.diff(off) >= 1).all() and z["line_verts"].shape == (V, nd)
    for name in ("line_origin", "line_manifold", "line_dim", "line_end", "line_target"):
        assert z[name].shape == (L,), name
    assert len(doc["steps"]) == K and z["offsets"][-1] == len(z["cell"])
    names = np.array(ops.critical_class_names(z["cls"], nd), dtype=object)
    saddle = "saddle" if nd == 2 else "saddle1"
    total = 0
    for j, row in enumerate(doc["steps"]):
        a, b = z["offsets"][j:j + 2]
        sel = np.nonzero(z["line_step"] == j)[0]
        assert len(sel) == lines_per_step == row["n_lines"] and (np.diff(sel) == 1).all()
        length = np.diff(off)[sel] - 1
        total += int((length + 1).sum())
        assert row["lines_by_end"] == {n: int((z["line_end"][sel] == i).sum()) for i, n in enumerate(ops.streamline_end_names)}
        assert row["max_length"] == length.max() and abs(row["mean_length"] - length.mean()) < 1e-9
        # one saddle per step, and its two unstable lines end in the two sinks
        assert row["n_points"] == 3 == b - a and row["saddles_seeded"] == 1
        # (in 3-D every point has the two equal eigenvalues -1, -1, which make Delta a rounding error: a "sink" or a
        # "spiral_sink", a "saddle1" or a "spiral_saddle1")
        is_saddle = np.array([n.endswith(saddle) for n in names[a:b]])
        assert is_saddle.sum() == 1 == sum(c for n, c in row["classes"].items() if n.endswith(saddle))
        is_sink = np.array([n.endswith("sink") for n in names[a:b]])
        assert is_sink.sum() == 2 and sum(row["connections"].values()) == 2 and row["saddle_connections"] == 0
        assert all(n.endswith("sink") for n in row["connections"])
        sad = a + int(np.nonzero(is_saddle)[0][0])
        sep = sel[z["line_manifold"][sel] < 2]
        assert (z["line_origin"][sep] == sad).all()
        un = sep[z["line_manifold"][sep] == 0]
        assert len(un) == 2 and (z["line_end"][un] == CAPTURED).all()
        tg = z["line_target"][un]
        assert sorted(tg.tolist()) == sorted((a + np.nonzero(is_sink)[0]).tolist())
        for i, t in zip(un, tg):  # the line ends in its sink's cell: within a cell's diagonal of the point
            assert np.abs(z["line_verts"][off[i + 1] - 1] - z["pos"][t]).max() < 1.0
        st = sep[z["line_manifold"][sep] == 1]
        assert (z["line_end"][st] == OUT).all() and (z["line_target"][st] == -1).all()
    assert total == V  # the sum of length + 1
    return V


def test_flow2d_main_draws_the_double_wells(tmp_path):
    shots = str(tmp_path / "shots")
    doc, z, c, s = _main(tmp_path, 2, ["--png-dir", shots, "--seed-grid", "3"])
    assert doc["shape"] == [33, 33] and doc["method"] == "rk4" and doc["seed_grid"] == 3 and doc["time_lines_s"] > 0
    _adds_up(doc, z, 2, 4 + 2 * 9)
    ctx = z["line_manifold"] == 2
    assert ctx.sum() == K * 18 and (z["line_origin"][ctx] == -1).all() and (z["line_dim"] == 1).all()
    names = sorted(os.listdir(shots))
    assert names == ["skeleton_%03d_to_%03d.png" % (r["t_from"], r["t_to"]) for r in doc["steps"]]
    assert doc["pngs"] == [os.path.join(shots, f) for f in names]
    for f in names:
        w, h, colour, rows = _png(os.path.join(shots, f))
        assert (w, h, colour) == (33, 33, 2) and rows.shape == (33, 3 * 33)
        img = rows.reshape(33, 33, 3)
        # the unstable lines run along y = 16.41 from the saddle to the sinks: red pixels between them, blue ones on the
        # stable line x = 16.3, and the saddle's green marker on top of both
        assert img[16, 12].tolist() == [255, 50, 40] and img[16, 20].tolist() == [255, 50, 40]
        assert img[8, 16].tolist() == [40, 90, 255] and img[25, 16].tolist() == [40, 90, 255]
        assert img[16, 16].tolist() == [40, 220, 60]
        assert (img.reshape(-1, 3) == [150, 150, 150]).all(1).sum() > 20  # context lines


def test_flow3d_main_writes_vtk_lines(tmp_path):
    lines = str(tmp_path / "lines")
    doc, z, c, s = _main(tmp_path, 3, ["--lines-dir", lines, "--surface-seeds", "6"])
    assert doc["shape"] == [21, 21, 21] and doc["surface_seeds"] == 6
    V = _adds_up(doc, z, 3, 2 + 6)
    assert sorted(np.unique(z["line_dim"]).tolist()) == [1, 2] and ((z["line_dim"] == 2) == (z["line_manifold"] == 1)).all()
    names = sorted(os.listdir(lines))
    assert names == ["skeleton_%03d_to_%03d.vtk" % (r["t_from"], r["t_to"]) for r in doc["steps"]]
    assert doc["vtks"] == [os.path.join(lines, f) for f in names]
    seen = 0
    for j, f in enumerate(names):
        tok = open(os.path.join(lines, f)).read().split("\n")
        assert tok[0].startswith("# vtk DataFile") and tok[2] == "ASCII" and tok[3] == "DATASET POLYDATA"
        kind, n, typ = tok[4].split()
        n = int(n)
        assert kind == "POINTS" and typ == "float"
        pts = np.array([[float(v) for v in line.split()] for line in tok[5:5 + n]], np.float32)
        sel = np.nonzero(z["line_step"] == j)[0]
        a, b = z["line_offsets"][sel[0]], z["line_offsets"][sel[-1] + 1]
        assert n == b - a and np.array_equal(pts, z["line_verts"][a:b])  # (repr of a float round-trips)
        head = tok[5 + n].split()
        assert head[0] == "LINES" and int(head[1]) == len(sel) and int(head[2]) == len(sel) + n
        at = 0
        for i, line in zip(sel, tok[6 + n:6 + n + len(sel)]):
            ids = [int(v) for v in line.split()]
            assert ids[0] == len(ids) - 1 == z["line_offsets"][i + 1] - z["line_offsets"][i] and ids[1:] == list(range(at, at + ids[0]))
            at += ids[0]
        rest = tok[6 + n + len(sel):]
        assert rest[0] == "CELL_DATA %d" % len(sel)
        for name, col in (("manifold", z["line_manifold"][sel]), ("end", z["line_end"][sel]),
                          ("target", np.where(z["line_target"][sel] >= 0, z["line_target"][sel] - z["offsets"][j], -1))):
            k = rest.index("SCALARS %s int 1" % name)
            assert rest[k + 1] == "LOOKUP_TABLE default"
            assert [int(v) for v in rest[k + 2:k + 2 + len(sel)]] == col.tolist(), name
        seen += n
    assert seen == V
