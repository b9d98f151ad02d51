"""TEST INFRASTRUCTURE -- toy cases and numpy restatements for the 2-D training loader tests."""
import types

import numpy as np


class ToyDataset:
    """nnUNetDataset-like: keys() and load_case(key) -> (data [C,D,H,W] float32, seg [1,D,H,W] int16, properties)."""

    def __init__(self, cases):
        self.cases = cases

    def keys(self):
        return list(self.cases.keys())

    def load_case(self, key):
        return self.cases[key]


def dataset_from_fixture(scen, random_values=False):
    """The toy cases of a tests/golden/loader2d.json scenario.  Channel 0 holds z + 1 (what the generator used); with
    random_values the voxels are random and the seg carries labels at the class locations."""
    rng = np.random.default_rng(7)
    cases = {}
    for key, c in scen["cases"].items():
        shape = tuple(c["shape"])
        cl = {(tuple(k) if isinstance(k, list) else k): np.asarray(v, dtype=np.int64).reshape(-1, 4)
              for k, v in c["class_locations"]}
        if random_values:
            data = rng.standard_normal((scen["channels"], *shape)).astype(np.float32)
            seg = np.zeros((1, *shape), dtype=np.int16)
            for k, v in cl.items():
                if not isinstance(k, tuple) and len(v):
                    seg[0, v[:, 1], v[:, 2], v[:, 3]] = k
        else:
            data = np.zeros((scen["channels"], *shape), dtype=np.float32)
            data[0] = (np.arange(shape[0], dtype=np.float32) + 1)[:, None, None]
            seg = np.zeros((1, *shape), dtype=np.int16)
        cases[key] = (data, seg, {"class_locations": cl})
    return ToyDataset(cases)


def label_manager(scen):
    return types.SimpleNamespace(all_labels=list(scen["all_labels"]), has_ignore_label=bool(scen["has_ignore"]))


def crop_pad_2d(data, seg, z, lbs, patch):
    """data_loader_2d.py:45-84 for one sample: slice z, crop to the valid part of the box, pad data with 0 and seg with -1."""
    d, s = data[:, z], seg[:, z]
    shape = d.shape[1:]
    ubs = [lbs[i] + patch[i] for i in range(2)]
    vl = [max(0, lbs[i]) for i in range(2)]
    vu = [min(shape[i], ubs[i]) for i in range(2)]
    padding = [(-min(0, lbs[i]), max(ubs[i] - shape[i], 0)) for i in range(2)]
    d = np.pad(d[:, vl[0]:vu[0], vl[1]:vu[1]], ((0, 0), *padding), 'constant', constant_values=0)
    s = np.pad(s[:, vl[0]:vu[0], vl[1]:vu[1]], ((0, 0), *padding), 'constant', constant_values=-1)
    return d, s
