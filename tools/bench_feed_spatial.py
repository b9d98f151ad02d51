"""Times the on-device SpatialTransform feed: batches of 2 x 4-channel 128^3 patches warped from 205^3 initial
patches of 160x224x192 cases, with every sample modified and with the reference probabilities (0.2 / 0.2).  Prints ms
per batch and the bytes counted from shapes."""
import time

import numpy as np
import torch

from multimodal_mvd_seg_amd.dataloading import DeviceDataLoader3D, get_patch_size


class _DS:
    def __init__(self, n, shape, channels=4):
        rng = np.random.default_rng(0)
        self.cases = {}
        for i in range(n):
            data = rng.standard_normal((channels, *shape)).astype(np.float32)
            seg = (rng.random((1, *shape)) > 0.95).astype(np.int16) * rng.integers(1, 5, (1, *shape)).astype(np.int16)
            locs = {c: np.argwhere(seg == c)[:10000] for c in (1, 2, 3, 4)}
            self.cases[f"c{i}"] = (data, seg, {"class_locations": locs})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


class _L:
    all_labels = [1, 2, 3, 4]
    has_ignore_label = False


def modified_bytes(C, n, f):
    """Counted traffic of one modified sample: crop (read + write of C+1 initial patches, seg read as int16), three
    prefilter passes (read + write), the warps (read the patches once, write C+1 final patches)."""
    nv, fv = int(np.prod(n)), int(np.prod(f))
    crop = C * nv * 8 + nv * (2 + 4)
    prefilter = 3 * C * nv * 8
    warp = (C + 1) * nv * 4 + (C + 1) * fv * 4
    return crop + prefilter + warp


def plain_bytes(C, f):
    fv = int(np.prod(f))
    return C * fv * 8 + fv * (2 + 4)


def run(dl, nbatches):
    plans = [dl.plan_batch() for _ in range(nbatches)]
    for p in plans[:3]:
        dl.generate_train_batch(p)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in plans:
        dl.generate_train_batch(p)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / len(plans) * 1e3
    nmod = sum(s is not None for p in plans for s in p[2])
    return ms, nmod / (len(plans) * dl.batch_size), plans


def main():
    f = (128, 128, 128)
    rot = {ax: (-np.pi / 6, np.pi / 6) for ax in 'xyz'}
    n = tuple(int(v) for v in get_patch_size(f, *rot.values(), (0.85, 1.25)))
    scales = [1, 0.5, 0.25, 0.125, 0.0625]
    ds = _DS(6, (160, 224, 192))
    C = 4
    for name, p in (("all-modified", 1.0), ("reference p=0.2/0.2", 0.2)):
        dl = DeviceDataLoader3D(ds, 2, n, f, _L(), oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2),
                                deep_supervision_scales=scales, device="cuda:0", rotation_for_DA=rot,
                                p_rot_per_sample=p, p_scale_per_sample=p)
        np.random.seed(0)
        for _ in range(6):
            next(dl)  # uploads every case once
        ms, frac, plans = run(dl, 40)
        nmod = frac * 2
        nbytes = nmod * modified_bytes(C, n, f) + (2 - nmod) * plain_bytes(C, f)
        print(f"{name}: {ms:.3f} ms per batch of 2 ({C}x{n[0]}^3 -> {f[0]}^3, 5 DS targets), "
              f"{frac * 100:.0f} % of samples modified, {nbytes / 1e9:.2f} GB counted per batch = "
              f"{nbytes / ms / 1e6:.0f} GB/s")


if __name__ == "__main__":
    main()
