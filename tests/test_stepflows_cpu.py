"""opticalflowscivis_amd/stepflows.py without a GPU and without a model: open_step_flows on the CPU with a fake model (the
parity trick of `source`), its --flows path, the four tools' parsers against the defaults written out here, the shared
bad command lines, the model loader with a stub Model, and write_report."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from opticalflowscivis_amd import ftle, regions, stepflows, trace, vortex
from opticalflowscivis_amd.rife import load_pretrained

TOOLS = {"trace": (trace, ["--seed-grid", "1"]), "ftle": (ftle, ["--window", "2"]), "vortex": (vortex, []),
         "regions": (regions, [])}
CONFIGS = ((2, "rife"), (3, "rife"), (2, "upflow"))


def _source_args(nd, model, argv):
    ap = argparse.ArgumentParser()
    stepflows.add_source_args(ap, nd, model, "d", "c")
    return stepflows.check_source_args(ap.parse_args(argv))


def _fake_model(T, gap, C, sp, calls):
    """make_model whose flows_of(frames, pairs) fills rows 2i and 2i + 1 with 2 * (index of pairs[i] in the series' pair
    list) + 0 / 1: what row of the full [2P, C, *sp] stack the model would have put there."""
    all_pairs = [(t, t + gap) for t in range(T - gap)]

    def make_model():
        calls.append("made")

        def flows_of(frames, pairs):
            assert frames.shape == (T,) + sp
            out = torch.empty((2 * len(pairs), C) + sp)
            for i, p in enumerate(pairs):
                out[2 * i] = 2 * all_pairs.index(p)
                out[2 * i + 1] = 2 * all_pairs.index(p) + 1
            return out
        return flows_of
    return make_model


@pytest.mark.parametrize("model,T,gap", [("rife", 9, 2), ("rife", 9, 4), ("upflow", 4, 1), ("upflow", 4, 2)])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("sp", [(5, 6), (3, 4, 5)])
def test_model_source_hands_out_the_chain_rows(tmp_path, model, T, gap, direction, sp):
    nd = len(sp)
    seq = str(tmp_path / "s.npy")
    np.save(seq, np.zeros((T,) + sp, np.float32))
    args = _source_args(nd, model, ["--seq", seq, "--gap", str(gap), "--direction", direction])
    calls = []
    sf = stepflows.open_step_flows(args, nd, model, _fake_model(T, gap, nd, sp, calls), "cpu")
    chain = stepflows.step_chain(T, gap, direction, model)
    assert chain and calls == ["made"]
    assert sf.name == "s.npy" and sf.sp == sp and sf.gt is None and tuple(sf.frames.shape) == (T,) + sp
    assert sf.n_steps == len(chain) and sf.visited == [chain[0][0]] + [c[1] for c in chain]
    n = 0
    for j0 in range(sf.n_steps):
        for j1 in range(j0 + 1, min(sf.n_steps, j0 + 3) + 1):
            got = sf.source(j0, j1)
            want = torch.stack([torch.full((nd,) + sp, float(chain[j][2])) for j in range(j0, j1)])
            assert got.shape == want.shape and torch.equal(got, want), (j0, j1)
            n += 1
    assert n >= 1 and calls == ["made"]  # one model for every chunk


def test_a_series_too_short_for_a_step_builds_no_model(tmp_path):
    seq = str(tmp_path / "s.npy")
    np.save(seq, np.zeros((3, 5, 6), np.float32))
    calls = []
    sf = stepflows.open_step_flows(_source_args(2, "rife", ["--seq", seq]), 2, "rife", _fake_model(3, 2, 2, (5, 6), calls), "cpu")
    assert sf.n_steps == 0 and sf.visited == [] and calls == [] and sf.sp == (5, 6)
    bad = str(tmp_path / "bad.npy")
    np.save(bad, np.zeros((3, 5), np.float32))
    with pytest.raises(SystemExit):  # --seq of the wrong rank
        stepflows.open_step_flows(_source_args(2, "rife", ["--seq", bad]), 2, "rife", None, "cpu")


def test_given_flows_as_an_array(tmp_path):
    rng = np.random.default_rng(0)
    arr = rng.standard_normal((3, 2, 5, 6)).astype(np.float32)
    path = str(tmp_path / "f.npy")
    np.save(path, arr)
    sf = stepflows.open_step_flows(_source_args(2, "rife", ["--flows", path]), 2, "rife", None, "cpu")
    assert sf.name == "f.npy" and sf.frames is None and sf.gt is None and sf.sp == (5, 6)
    assert sf.visited == [0, 1, 2, 3] and sf.n_steps == 3
    got = sf.source(0, 3)
    assert got.dtype == torch.float32 and got.device.type == "cpu" and np.array_equal(got.numpy(), arr)
    assert np.array_equal(sf.source(1, 2).numpy(), arr[1:2])
    sf = stepflows.open_step_flows(_source_args(2, "upflow", ["--flows", path, "--direction", "bwd", "--start", "3"]),
                                   2, "upflow", None, "cpu")
    assert sf.visited == [3, 2, 1, 0] and sf.n_steps == 3 and np.array_equal(sf.source(0, 3).numpy(), arr)
    with pytest.raises(SystemExit):  # frames would go negative
        stepflows.open_step_flows(_source_args(2, "rife", ["--flows", path, "--direction", "bwd", "--start", "2"]),
                                  2, "rife", None, "cpu")
    for shape in ((3, 2, 5), (3, 3, 5, 6), (0, 2, 5, 6)):  # a wrong rank, a wrong channel count, no flow at all
        np.save(path, np.zeros(shape, np.float32))
        with pytest.raises(SystemExit):
            stepflows.open_step_flows(_source_args(2, "rife", ["--flows", path]), 2, "rife", None, "cpu")


def test_given_flows_as_a_directory(tmp_path):
    d = str(tmp_path / "flows")
    os.mkdir(d)
    # the file set of test_advect_cpu.test_flow_directory_chaining, every file filled with 10 * from + to
    for a, b in ((1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 4), (3, 6)):
        np.save(os.path.join(d, "flow_%03d_to_%03d.npy" % (a, b)), np.full((2, 3, 3), 10 * a + b, np.float64))
    open(os.path.join(d, "class_001_to_002.npy"), "w").close()
    sf = stepflows.open_step_flows(_source_args(2, "rife", ["--flows", d + "/", "--start", "1"]), 2, "rife", None, "cpu")
    assert sf.name == "flows" and sf.sp == (3, 3) and sf.visited == [1, 2, 3, 4] and sf.n_steps == 3
    got = sf.source(0, 3)
    assert got.dtype == torch.float32 and got.shape == (3, 2, 3, 3) and got[:, 0, 0, 0].tolist() == [12, 23, 34]
    assert sf.source(2, 3)[:, 1, 2, 2].tolist() == [34]
    sf = stepflows.open_step_flows(_source_args(2, "rife", ["--flows", d, "--start", "3", "--direction", "bwd"]),
                                   2, "rife", None, "cpu")
    assert sf.visited == [3, 2, 1, 0] and sf.source(0, 3)[:, 0, 0, 0].tolist() == [32, 21, 10]
    with pytest.raises(SystemExit):  # nothing leads forward from frame 0
        stepflows.open_step_flows(_source_args(2, "rife", ["--flows", d]), 2, "rife", None, "cpu")
    with pytest.raises(SystemExit):  # [2,3,3] files are no 3-D flows
        stepflows.open_step_flows(_source_args(3, "rife", ["--flows", d, "--start", "1"]), 3, "rife", None, "cpu")


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_flows_beside_a_series_of_another_extent_are_refused_by_every_tool(tmp_path, tool):
    mod, own = TOOLS[tool]
    flows, seq, other = (str(tmp_path / n) for n in ("f.npy", "s.npy", "o.npy"))
    np.save(flows, np.zeros((3, 2, 5, 6), np.float32))
    np.save(seq, np.zeros((4, 5, 6), np.float32))
    np.save(other, np.zeros((4, 5, 7), np.float32))
    parse = lambda s: mod.check_args(mod._args(2, "x", "rife").parse_args(["--flows", flows, "--seq", s] + own))
    sf = stepflows.open_step_flows(parse(seq), 2, "rife", None, "cpu")
    assert tuple(sf.frames.shape) == (4, 5, 6) and sf.visited == [0, 1, 2, 3]
    with pytest.raises(SystemExit) as e:
        stepflows.open_step_flows(parse(other), 2, "rife", None, "cpu")
    assert str(e.value) == "the flows' extent (5, 6) is not the series' (5, 7)"


@pytest.mark.parametrize("tool", sorted(TOOLS))
@pytest.mark.parametrize("nd,model", CONFIGS)
def test_parser_defaults(tool, nd, model):
    mod, own = TOOLS[tool]
    a = mod.check_args(mod._args(nd, "x", model).parse_args(["--flows", "f.npy"] + own))
    assert a.gap == (1 if model == "upflow" else 2)
    assert (a.chunk, a.batch, a.start, a.frames, a.seed, a.direction, a.model) == (4, 1, 0, 9, 1234, "fwd", "train_log")
    assert (a.dataset, a.seq, a.flows, a.size, a.json) == (None, None, "f.npy", None, None)
    if tool != "trace":
        assert a.dt == 1.0
    if tool in ("vortex", "regions"):
        assert a.spacing == [1.0] and a.nd == nd and a.save_flows is None
    with_model = mod._args(nd, "x", model).parse_args(["--dataset", "droplet3d" if nd == 3 else "rectangle2d", "--gap", "4",
                                                       "--size", "8", "12", "--batch", "3"] + own)
    assert (with_model.gap, with_model.size, with_model.batch) == (4, [8, 12], 3)


@pytest.mark.parametrize("tool", sorted(TOOLS))
@pytest.mark.parametrize("nd,model", CONFIGS)
def test_shared_bad_command_lines(tool, nd, model):
    mod, own = TOOLS[tool]
    ds = "droplet3d" if nd == 3 else "droplet2d"
    bad = [[],                                                  # no source
           ["--dataset", ds, "--seq", "s.npy"],                 # two series
           ["--flows", "f.npy", "--start", "-1"],
           ["--dataset", ds, "--chunk", "0"],
           ["--dataset", ds, "--batch", "0"]]
    if tool != "trace":
        bad += [["--dataset", ds, "--dt", v] for v in ("0", "-1", "inf", "nan")]
    if tool in ("vortex", "regions"):
        bad += [["--dataset", ds, "--spacing"] + v for v in (["1"] * (nd + 1), ["1", "2"] if nd == 3 else ["1"] * 4, ["0"],
                                                            ["inf"])]
    for argv in bad:
        args = mod._args(nd, "x", model).parse_args(argv + own)
        with pytest.raises(SystemExit):
            mod.check_args(args)
    for argv in (["--dataset", "rectangle2d" if nd == 3 else "droplet3d"], ["--dataset", ds, "--direction", "up"]):
        with pytest.raises(SystemExit):  # refused by the parser itself
            mod._args(nd, "x", model).parse_args(argv + own)


class _StubModel:
    def __init__(self, local_rank, device=None):
        self.made, self.loaded, self.evals = (local_rank, device), [], 0

    def load_model(self, name, path):
        self.loaded.append((name, path))
        if path == "nowhere":
            raise FileNotFoundError(path)

    def eval(self):
        self.evals += 1


def test_load_pretrained(capsys):
    m = load_pretrained(_StubModel, "nowhere", "cpu")
    assert isinstance(m, _StubModel) and m.made == (-1, "cpu") and m.loaded == [("flownet.pkl", "nowhere")] and m.evals == 1
    assert capsys.readouterr().out == "no flownet.pkl under nowhere: using random-init weights\n"
    m = load_pretrained(_StubModel, "somewhere", "cpu")
    assert m.loaded == [("flownet.pkl", "somewhere")] and m.evals == 1 and capsys.readouterr().out == ""
    # the tools' factory: the same loader, and nothing is built before make_model() is called
    made = []

    class Recording(_StubModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    make_model = stepflows.rife_model(Recording, argparse.Namespace(model="nowhere", batch=1))
    assert made == []
    assert callable(make_model()) and len(made) == 1 and made[0].evals == 1 and made[0].made == (-1, torch.device("cuda"))
    assert capsys.readouterr().out == "no flownet.pkl under nowhere: using random-init weights\n"
    nets = []
    assert callable(stepflows.upflow_model(nets.append, argparse.Namespace(model="w.pkl", batch=2))()) and nets == ["w.pkl"]


def test_write_report(tmp_path):
    doc = {"a": [1, 2], "b": {"c": None}}
    js, one, two = (str(tmp_path / d / n) for d, n in (("r", "r.json"), ("x/y", "one.npy"), ("z", "two.npy")))
    made = []
    stepflows.write_report(doc, js, {one: np.arange(3), two: lambda: made.append(1) or np.ones(2), None: lambda: 1 / 0})
    assert open(js).read() == json.dumps(doc, indent=1) and made == [1]
    assert np.load(one).tolist() == [0, 1, 2] and np.load(two).tolist() == [1, 1]
    stepflows.write_report(doc, None)  # nothing to write
    stepflows.write_report(doc, None, {None: lambda: 1 / 0})
    assert sorted(os.listdir(str(tmp_path))) == ["r", "x", "z"]
