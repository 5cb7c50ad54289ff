"""Generates tests/golden/series_rectangle3d.npz by RUNNING THE REFERENCE's Flow-3D/load_datasets.py `load_data`.

Build-container only (needs the reference tree; run by hand, never by the tests):

    python tests/golden/make_series_golden.py /path/to/reference

A small uint8 [900,4,4,4] series is pickled as ../Datasets/rectangle3d.pkl relative to a temporary working directory
(where load_data looks for it), load_data("rectangle3d", "train") cuts it, and the input plus every 7th train /
validation item are stored.  Modules the reference imports at module scope but never uses in load_data (cv2, skimage,
matplotlib, turtle, its own utils) are replaced by inert stubs.
"""
import importlib.util
import os
import pickle
import sys
import tempfile
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def _stub(name):
    m = types.ModuleType(name)
    m.__getattr__ = lambda k: (_ for _ in ()).throw(AttributeError(k)) if k.startswith("__") else (lambda *a, **kw: None)
    sys.modules[name] = m


def main(ref):
    for name in ("turtle", "cv2", "matplotlib", "matplotlib.pyplot", "skimage", "skimage.transform", "utils"):
        _stub(name)
    rng = np.random.default_rng(20240607)
    data = rng.integers(0, 256, size=(900, 4, 4, 4), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Datasets"))
        os.makedirs(os.path.join(tmp, "run"))
        with open(os.path.join(tmp, "Datasets", "rectangle3d.pkl"), "wb") as f:
            pickle.dump(data, f)
        spec = importlib.util.spec_from_file_location("ref_load_datasets", os.path.join(ref, "Flow-3D", "load_datasets.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        cwd = os.getcwd()
        os.chdir(os.path.join(tmp, "run"))
        try:
            train, val = mod.load_data("rectangle3d", "train")
        finally:
            os.chdir(cwd)
    idx_t, idx_v = np.arange(0, len(train), 7), np.arange(0, len(val), 7)
    np.savez_compressed(os.path.join(OUT, "series_rectangle3d.npz"), data=data, n_train=len(train), n_val=len(val),
                        train_idx=idx_t, train=np.stack([np.asarray(train[i]) for i in idx_t]),
                        val_idx=idx_v, val=np.stack([np.asarray(val[i]) for i in idx_v]))
    print("train items", len(train), "val items", len(val), "stored", len(idx_t), len(idx_v))


if __name__ == "__main__":
    main(sys.argv[1])
