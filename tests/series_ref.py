"""Plain-numpy restatement of how the reference turns a stored array into training triplets
(Flow-3D/load_datasets.py:136-190), used by the series tests as the expected value."""
import numpy as np


def ref_triplets(data, n_train, n_total=None, cut=True):
    """data: [T,D,H,W] / [T,1,D,H,W] (a series, cut=True) or [N,3,D,H,W] (ready-made triplets, cut=False).
    Returns (train, val): arrays [items,3,D,H,W] in float32, as load_data builds them."""
    data = np.float32(data)                                              # load_datasets.py:95
    if data.ndim == 4:
        data = np.expand_dims(data, axis=1)                              # :97-98
    n_total = data.shape[0] if n_total is None else n_total
    data_train, data_val = data[:n_train], data[n_train:n_total]         # :138-139
    data_train = np.append(data_train, data_train[:, :, :, ::-1, :], axis=0)   # :149-150  (H mirrored copies)
    data_train = np.append(data_train, data_train[:, :, ::-1, :, :], axis=0)   # :151-152  (D mirrored copies)
    if cut:
        def three(a):                                                    # :172-176, :179-183
            return np.array([np.concatenate((a[i], a[i + 2], a[i + 1]), axis=0) for i in range(0, a.shape[0], 3)])
        data_train, data_val = three(data_train), three(data_val)
    return data_train, data_val
