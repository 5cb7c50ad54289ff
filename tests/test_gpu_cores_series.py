"""-m gpu: the `cores` driver.  core_fields forms the operands the host evaluation forms; cores_series on the ring
repeated over three steps finds one closed line per step, the same whatever the chunk; and `python -m
opticalflowscivis_amd.flow3d.cores --flows ...` in a child process writes a report whose rows match the .npz and VTK
line files that parse back to the same vertices."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pv_fields as F
import pv_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
CRITERIA = ("sujudi-haimes", "levy")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _ring_flows():
    return np.stack([F.ring()] * K)


@pytest.mark.parametrize("criterion", CRITERIA)
def test_core_fields_against_the_host_evaluation(criterion):
    from opticalflowscivis_amd import cores
    flows = np.stack([F.ring(), F.ring() * np.float32(0.5)])
    kw = dict(spacing=(1.0, 0.5, 2.0), scale=[1.0, 0.3])
    got = cores.core_fields(torch.from_numpy(flows).cuda(), criterion, **kw)
    v, w, q, l2 = F.core_fields(flows, criterion, **kw)
    for name, want in (("v", v), ("w", w), ("q", q)):
        g = got[name].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == want.shape and np.array_equal(_bits(g), _bits(want)), name
    assert got["l2"].shape == l2.shape and np.abs(got["l2"].cpu().numpy() - l2).max() < 1e-5
    with pytest.raises(ValueError):
        cores.core_fields(torch.from_numpy(flows).cuda(), "q")


@pytest.mark.parametrize("criterion", CRITERIA)
def test_series_on_the_ring_is_the_same_whatever_the_chunk(criterion):
    from opticalflowscivis_amd import cores
    flows = torch.from_numpy(_ring_flows()).cuda()
    asked = []

    def source(j0, j1):
        asked.append((j0, j1))
        return flows[j0:j1]

    a = cores.cores_series(source, K, flows.shape[2:], criterion, chunk=2, filt="q")
    assert asked == [(0, 2), (2, 3)]
    b = cores.cores_series(source, K, flows.shape[2:], criterion, chunk=1, filt="q")
    v, w, q, _ = F.core_fields(_ring_flows()[:1], criterion)
    want = R.parallel_vectors(v, w, q)
    keep = (want["aux"] > 0).all(1)
    for j in range(K):
        for c in cores.COLUMNS:
            assert np.array_equal(_bits(a["tables"][j][c]), _bits(b["tables"][j][c])), (j, c)
            assert np.array_equal(_bits(a["tables"][j][c]), _bits(want[c][keep])), (j, c)
        for c in ("verts", "offsets", "closed", "mu"):
            assert np.array_equal(_bits(a["lines"][j][c]), _bits(b["lines"][j][c])), (j, c)
        row = a["steps"][j]
        assert row == b["steps"][j]
        assert (row["n_found"], row["n_segments"], row["n_lines"], row["closed_lines"], row["open_ends"]) == \
            (int(want["counts"][0, 0]), 78, 1, 1, 0)
        assert row["ambiguous_tets"] == want["counts"][0, 1] and row["degenerate_faces"] == 0 and row["nonfinite_cells"] == 0
        assert 0.8 * 2 * np.pi * 4 < row["length"] < 2 * np.pi * 4 and np.isfinite(row["mean_mu"])
    # without the filter the locus also runs outside the vortex; a long minimum length drops its short pieces
    c = cores.cores_series(source, 1, flows.shape[2:], criterion, filt="none", min_vertices=40)
    assert c["steps"][0]["n_segments"] == c["steps"][0]["n_found"] >= 78 and c["steps"][0]["n_lines"] >= 1
    assert (np.diff(c["lines"][0]["offsets"]) >= 40).all()


def _vtk(path):
    tok = open(path).read().split("\n")
    assert tok[0].startswith("# vtk DataFile") and tok[2] == "ASCII" and tok[3] == "DATASET POLYDATA"
    kind, n, typ = tok[4].split()
    n = int(n)
    assert kind == "POINTS" and typ == "float"
    pts = np.array([[float(x) for x in line.split()] for line in tok[5:5 + n]], np.float32).reshape(n, 3)
    head = tok[5 + n].split()
    assert head[0] == "LINES"
    L = int(head[1])
    lines = [[int(x) for x in line.split()] for line in tok[6 + n:6 + n + L]]
    assert int(head[2]) == L + n and all(l[0] == len(l) - 1 for l in lines)
    rest = tok[6 + n + L:]
    assert rest[0] == "CELL_DATA %d" % L
    k = rest.index("SCALARS end int 1")
    return pts, lines, [int(x) for x in rest[k + 2:k + 2 + L]]


def test_flow3d_cores_in_a_child_process(tmp_path):
    fl, out, rep, lines = (str(tmp_path / n) for n in ("flows.npy", "cores.npz", "r.json", "lines"))
    np.save(fl, _ring_flows() * np.array([1.0, 2.0, 4.0], np.float32)[:, None, None, None, None])
    r = subprocess.run([sys.executable, "-m", "opticalflowscivis_amd.flow3d.cores", "--flows", fl, "--chunk", "2",
                        "--criterion", "levy", "--filter", "q", "--out", out, "--lines-dir", lines, "--json", rep],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    doc = json.load(open(rep))
    z = dict(np.load(out))
    assert doc["shape"] == list(F.RING["shape"]) and doc["criterion"] == "levy" and len(doc["steps"]) == K
    names = sorted(os.listdir(lines))
    assert names == ["cores_%03d_to_%03d.vtk" % (w["t_from"], w["t_to"]) for w in doc["steps"]]
    assert doc["vtks"] == [os.path.join(lines, f) for f in names]
    N = len(z["cell"])
    assert z["offsets"][-1] == N and z["key"].shape == (N, 2) and z["pos"].shape == (N, 2, 3) and z["mu"].dtype == np.float64
    assert z["line_offsets"][-1] == len(z["line_verts"]) == len(z["line_mu"])
    for j, row in enumerate(doc["steps"]):
        assert (row["n_lines"], row["closed_lines"], row["open_ends"], row["n_segments"]) == (1, 1, 0, 78)
        assert z["offsets"][j + 1] - z["offsets"][j] == row["n_segments"]
        sel = np.nonzero(z["line_step"] == j)[0]
        assert len(sel) == row["n_lines"] and z["line_closed"][sel].sum() == row["closed_lines"]
        pts, ls, end = _vtk(os.path.join(lines, names[j]))
        a, b = z["line_offsets"][sel[0]], z["line_offsets"][sel[-1] + 1]
        assert np.array_equal(pts, z["line_verts"][a:b])  # (repr of a float round-trips)
        assert len(ls) == row["n_lines"] and ls[0][1:] == list(range(79)) and end == [1]
        assert np.array_equal(pts[0], pts[-1])
        # the same loop at every step: the velocity doubles (exactly, in every operation), and mu = curl v / v does not change
        assert np.array_equal(pts, z["line_verts"][:79])
    assert abs(doc["steps"][0]["mean_mu"] - doc["steps"][2]["mean_mu"]) < 1e-3 * abs(doc["steps"][0]["mean_mu"])
    assert "1 lines (1 closed, 0 open ends)" in r.stdout
