"""Generates tests/golden/flow2rgb.npz by RUNNING THE REFERENCE's two `flow2rgb` functions (utils.py: the picture starts
black; Flow-3D/train.py: it starts white).

Build-container only (needs the reference tree; run by hand, never by the tests):

    python tests/golden/make_flow2rgb_golden.py /path/to/reference

The modules import plotting libraries at module scope that the function does not use, so only the function's own
definition is compiled out of each file (ast) and run with numpy in scope.  Inputs: a seeded random [7, 9, 2] flow, one
with a single dominant vector, and one with negative components only.
"""
import ast
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def _function(path, name):
    tree = ast.parse(open(path).read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    scope = {"np": np}
    exec(compile(ast.Module([node], []), path, "exec"), scope)
    return scope[name]


def main(ref):
    rng = np.random.default_rng(20241020)
    a = rng.normal(size=(7, 9, 2)).astype(np.float32)
    b = (0.1 * rng.normal(size=(5, 4, 2))).astype(np.float32)
    b[2, 1] = (3.0, -4.0)
    c = -np.abs(rng.normal(size=(3, 6, 2))).astype(np.float32)
    black = _function(os.path.join(ref, "utils.py"), "flow2rgb")
    white = _function(os.path.join(ref, "Flow-3D", "train.py"), "flow2rgb")
    out = {}
    for n, x in (("a", a), ("b", b), ("c", c)):
        out["in_" + n] = x
        out["black_" + n] = black(x.copy())
        out["white_" + n] = white(x.copy())
    np.savez_compressed(os.path.join(OUT, "flow2rgb.npz"), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
