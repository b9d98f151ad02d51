"""Times the on-device DA5 stage of the feed: batches of 2 x 4-channel 128^3 patches cut from 160x224x192
cases with the stage off, with DA5 at the reference probabilities, and with every transform on every sample and channel
("all-on").  Then every new kernel alone on one 4 x 128^3 sample, and the median kernel alone at s = 2, 3, 5, 7 on one
128^3 channel next to scipy.ndimage.median_filter on the same volume on the host.  Prints ms."""
import argparse
import time

import numpy as np
import torch
from scipy import ndimage

from multimodal_mvd_seg_amd import dataloading as DLD

DEV = "cuda:0"


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


def run(dl, nbatches):
    plans = [dl.plan_batch() for _ in range(nbatches)]
    for p in plans[:3]:
        dl.generate_train_batch(p)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in plans:
        dl.generate_train_batch(p)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(plans) * 1e3


def timed(fn, reps=10):
    """Median of `reps` event-timed calls after two warm-up calls, in ms."""
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def kernels():
    C, f = 4, (128, 128, 128)
    x = torch.randn((C, *f), device=DEV)
    y = torch.empty_like(x)
    st = torch.empty((C, 4), dtype=torch.float64, device=DEV)
    sws = DLD.stats_workspace(C, DEV)
    DLD.channel_stats(x, st, sws)
    ws2 = torch.empty(2 * C * x[0].numel(), dtype=torch.float32, device=DEV)
    rect = torch.empty(DLD.RECT_WS_DOUBLES, dtype=torch.float64, device=DEV)
    loc = [([30., 50., 80.], [40., -20., 150.], 3.0)] * C
    rows = [("channel_stats, 4 channels", lambda: DLD.channel_stats(x, st, sws)),
            ("signed_permute, W kept (mirror)", lambda: DLD.signed_permute(x, y, (0, 1, 2), 5)),
            ("signed_permute, W moved", lambda: DLD.signed_permute(x, y, (2, 0, 1), 3)),
            ("gaussian_blur_wide, sigma 1.5, 4 channels", lambda: DLD.gaussian_blur_wide(x, [1.5] * C, ws2)),
            ("additive brightness", lambda: DLD.da5_apply(x, DLD.OP_DA5_ADD, [0.1] * C)),
            ("contrast, no clip", lambda: DLD.da5_apply(x, DLD.OP_DA5_CONTRAST_NOCLIP, [1.1] * C, st)),
            ("blank_rectangle, 42^3 box", lambda: DLD.blank_rectangle(x, 0, (10, 20, 30), (42, 42, 42), rect)),
            ("local_gauss additive, 4 channels", lambda: DLD.local_gauss(x, DLD.LOCAL_ADDITIVE, loc)),
            ("local_gauss gamma, 4 channels", lambda: DLD.local_gauss(x, DLD.LOCAL_GAMMA, loc, st)),
            ("sharpen, 4 channels", lambda: DLD.sharpen(x, y, [0.5] * C, st))]
    for s in (2, 3, 5, 7):
        rows.append((f"median_filter s = {s}, 4 channels", lambda s=s: DLD.median_filter(x, y, [s] * C)))
    for name, fn in rows:
        print(f"kernel {name}: {timed(fn):.3f} ms")


def median_alone(host):
    vol = np.random.default_rng(1).standard_normal((1, 128, 128, 128)).astype(np.float32)
    x = torch.from_numpy(vol).to(DEV)
    y = torch.empty_like(x)
    for s in (2, 3, 5, 7):
        ms = timed(lambda: DLD.median_filter(x, y, [s]))
        line = f"median s = {s}, one 128^3 channel: device {ms:.3f} ms"
        if host:
            t0 = time.perf_counter()
            ref = ndimage.median_filter(vol[0], size=s, mode='reflect')
            hs = (time.perf_counter() - t0) * 1e3
            line += f", scipy on the host {hs:.0f} ms ({hs / ms:.0f}x), equal: {np.array_equal(y[0].cpu().numpy(), ref)}"
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--modes", default="off,reference,all-on")
    ap.add_argument("--no-host", action="store_true", help="skip scipy's median on the host")
    args = ap.parse_args()
    f = (128, 128, 128)
    C = 4
    scales = [1, 0.5, 0.25, 0.125, 0.0625]
    ds = _DS(6, (160, 224, 192), C)
    modes = {"off": {}, "reference": dict(da5=True),
             "all-on": dict(da5=True, da5_probabilities={k: 1.0 for k in DLD.DA5_PROBABILITIES})}
    times = {}
    for name in args.modes.split(","):
        dl = DLD.DeviceDataLoader3D(ds, 2, f, f, _L(), oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2),
                                    deep_supervision_scales=scales, device=DEV, **modes[name])
        np.random.seed(0)
        for _ in range(6):
            next(dl)  # uploads every case once
        times[name] = run(dl, args.batches)
        extra = f" ({times[name] - times['off']:+.3f} ms vs off)" if "off" in times and name != "off" else ""
        print(f"{name}: {times[name]:.3f} ms per batch of 2 ({C}x{f[0]}^3, 5 DS targets, {args.batches} batches){extra}")
    kernels()
    median_alone(not args.no_host)


if __name__ == "__main__":
    main()
