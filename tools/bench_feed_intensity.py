"""Times the on-device intensity stage of the feed: batches of 2 x 4-channel 128^3 patches cut from
160x224x192 cases, with every intensity transform on every sample and channel ("all-on"), with the reference
probabilities, and with the stage off.  The stage's cost is a mode's time minus the off time.  Prints ms per batch and
the bytes counted from shapes."""
import argparse
import time

import numpy as np
import torch

from multimodal_mvd_seg_amd.dataloading import LOWRES_PAD, DeviceDataLoader3D, lowres_target_shape

ALL_ON = dict(p_noise=1.0, p_blur=1.0, p_blur_per_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_lowres=1.0,
              p_lowres_per_channel=1.0, p_gamma_inverted=1.0, p_gamma=1.0)


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


def intensity_bytes(it, C, f):
    """HBM traffic of one sample's intensity stage, counted from shapes: 8 B per voxel for a read-modify-write pass,
    4 B for a read-only statistics pass."""
    V = int(np.prod(f))
    n = 0
    if it['noise'] is not None:
        n += 8 * C * V
    if it['blur'] is not None:
        n += 3 * 8 * V * sum(s is not None for s in it['blur'])       # three separable passes
    if it['brightness'] is not None:
        n += 8 * C * V
    if it['contrast'] is not None:
        n += 4 * C * V + 8 * C * V                                    # statistics, apply
    for z in (it['lowres'] or []):
        if z is None:
            continue
        t = lowres_target_shape(f, z)
        P = int(np.prod([v + 2 * LOWRES_PAD for v in t]))
        n += 4 * int(np.prod(t)) + 4 * P                              # gather (read the samples, write the pad)
        n += 4 * P + 3 * 8 * P                                        # statistics, three prefilter passes
        n += 4 * P + 4 * V + 8 * V                                    # warp (read once, write), clip
    for key in ('gamma_inverted', 'gamma'):
        if it[key] is not None:
            n += 2 * 4 * C * V + 8 * C * V                            # statistics of x and of y, apply
    return n


def run(dl, nbatches):
    plans = [dl.plan_batch() for _ in range(nbatches)]
    for p in plans[:3]:
        dl.generate_train_batch(p)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in plans:
        dl.generate_train_batch(p)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(plans) * 1e3, plans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--modes", default="all-on,reference,off")
    args = ap.parse_args()
    f = (128, 128, 128)
    C = 4
    scales = [1, 0.5, 0.25, 0.125, 0.0625]
    ds = _DS(6, (160, 224, 192), C)
    modes = {"all-on": dict(intensity_augmentation=True, **ALL_ON), "reference": dict(intensity_augmentation=True),
             "off": {}}
    times = {}
    for name in args.modes.split(","):
        dl = DeviceDataLoader3D(ds, 2, f, f, _L(), oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2),
                                deep_supervision_scales=scales, device="cuda:0", **modes[name])
        np.random.seed(0)
        for _ in range(6):
            next(dl)  # uploads every case once
        ms, plans = run(dl, args.batches)
        times[name] = ms
        its = [it for p in plans if len(p) == 5 for it in p[3]]
        nbytes = sum(intensity_bytes(it, C, f) for it in its) / len(plans)
        extra = f" ({ms - times['off']:+.3f} ms vs off)" if "off" in times and name != "off" else ""
        print(f"{name}: {ms:.3f} ms per batch of 2 ({C}x{f[0]}^3, 5 DS targets, {len(plans)} batches){extra}, "
              f"intensity stage {nbytes / 1e9:.3f} GB counted per batch")
    if "off" in times:
        for name in times:
            if name != "off":
                print(f"{name}: intensity stage {times[name] - times['off']:.3f} ms per batch")


if __name__ == "__main__":
    main()
