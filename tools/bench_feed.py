"""Times the on-device training feed (SURVEY 8f-2 slice) at the BASELINE cfg-2 batch shape and the numpy oracle
(the reference's per-batch CPU work without the batchgenerators intensity transforms) beside it.

`--dummy2d` times the in-plane (dummy 2-D) path at the author's anisotropic shape instead (patch
64x128x256, initial patch 64x301x301, 2 channels, batch 2): one modified sample and one low-resolution channel
through the dedicated 2-D kernels and, on the same buffers, through the embedded-affine 3-D kernels (prefilter mask 7,
spatial_affine((a, 0, 0, sc)) with the z row set to the identity; low-res with t[0] = D), then whole batches of the
dummy-2-D loader.  HIP events, warm-up, median of alternating repeats."""
import sys
import time

import numpy as np
import torch

from multimodal_mvd_seg_amd import dataloading as DLD
from multimodal_mvd_seg_amd.dataloading import DeviceDataLoader3D


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


def main():
    patch = (128, 128, 128)
    scales = [1, 0.5, 0.25, 0.125, 0.0625]
    ds = _DS(6, (160, 224, 192))
    dl = DeviceDataLoader3D(ds, 2, patch, patch, _L(), oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2),
                            deep_supervision_scales=scales, device="cuda:0")
    np.random.seed(0)
    for _ in range(6):
        next(dl)  # uploads every case once
    torch.cuda.synchronize()
    plans = [dl.plan_batch() for _ in range(50)]
    t0 = time.perf_counter()
    for p in plans:
        b = dl.generate_train_batch(p)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / len(plans) * 1e3
    nbytes = 2 * (4 + 1) * 128 ** 3 * 4 * 2  # read + write of data and target, per batch
    print(f"device feed: {ms:.3f} ms per batch of 2 (4x128^3 + 5 DS targets) = {2 / ms * 1e3:.0f} samples/s, "
          f"{nbytes / ms / 1e6:.0f} GB/s of batch traffic")
    if "--cpu" in sys.argv:
        sys.path.insert(0, ".")
        from oracle import feed_oracle as FO
        cases = {k: (v[0], v[1]) for k, v in ds.cases.items()}
        t0 = time.perf_counter()
        for p in plans[:5]:
            FO.generate_train_batch(cases, p[0], p[1], p[2], patch, scales)
        cpu_ms = (time.perf_counter() - t0) / 5 * 1e3
        print(f"numpy oracle (one core): {cpu_ms:.1f} ms per batch")


def _event_ms(fn, warmup=5, repeats=30):
    """Per-repeat HIP-event times (ms) of each callable of `fn`, alternating between them."""
    for _ in range(warmup):
        for f in fn:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fn]
    for _ in range(repeats):
        for i, f in enumerate(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [np.array(t) for t in times]


def _row(name, t):
    med = float(np.median(t))
    lo, hi = np.percentile(t, [10, 90])
    print(f"  {name:<44s} median {med:8.3f} ms   p10 {lo:8.3f}   p90 {hi:8.3f}   spread (p90-p10)/median "
          f"{(hi - lo) / med * 100:5.1f} %")
    return med, (hi - lo) / med


def dummy2d():
    dev = torch.device("cuda:0")
    n, f, C = (64, 301, 301), (64, 128, 256), 2
    g = torch.Generator(device="cpu").manual_seed(0)
    src = torch.randn((C, *n), generator=g).to(dev)
    pseg = torch.randint(-1, 5, (1, *n), generator=g).float().to(dev)
    pdata = torch.empty_like(src)
    out = torch.empty((C, *f), device=dev)
    tseg = torch.empty((1, *f), device=dev)
    spatial, flip = (0.7, 0., 0., 0.9), 5
    aff2 = DLD.spatial_affine_2d(spatial, n[1:])
    aff3 = DLD.spatial_affine(spatial, n)
    aff3[0:3] = [1., 0., 0.]  # the z row: identity (scaling acts in-plane only)
    aff3[3], aff3[6] = 0., 0.

    def dedicated():
        pdata.copy_(src)
        DLD.bspline_prefilter(pdata, 6)
        DLD.spatial_transform_data_2d(pdata, out, aff2, flip, 0.0)
        DLD.spatial_transform_seg_2d(pseg, tseg, aff2, flip, replace=(-1, 0))

    def embedded():
        pdata.copy_(src)
        DLD.bspline_prefilter(pdata, 7)
        DLD.spatial_transform_data(pdata, out, aff3, flip, 0.0)
        DLD.spatial_transform_seg(pseg, tseg, aff3, flip, replace=(-1, 0))

    dedicated()
    o2, s2 = out.clone(), tseg.clone()
    embedded()
    print(f"dummy 2-D, modified sample {C}x{n[0]}x{n[1]}x{n[2]} -> {f[0]}x{f[1]}x{f[2]} (+ seg): max |data 2-D - 3-D| = "
          f"{float((o2 - out).abs().max()):.2e}, seg voxels that differ = {int((s2 != tseg).sum())}")
    td, te = _event_ms([dedicated, embedded])
    md, _ = _row("dedicated (prefilter 6 + warp2d data/seg)", td)
    me, se = _row("embedded-affine 3-D (prefilter 7 + warp data/seg)", te)
    print(f"  dedicated / embedded = {md / me:.3f} (allowed: 1 + max(3 %, baseline spread {se * 100:.1f} %))")

    # one low-resolution channel at zoom 0.75
    x = torch.randn((1, *f), generator=g).to(dev)
    xin = x.clone()
    st = torch.empty((1, 4), dtype=torch.float64, device=dev)
    ws = DLD.stats_workspace(1, dev)
    t = DLD.lowres_target_shape(f, 0.75)
    t[0] = f[0]
    P = DLD.LOWRES_PAD
    d2 = torch.empty((1, f[0], t[1] + 2 * P, t[2] + 2 * P), device=dev)
    d3 = torch.empty((1, *[v + 2 * P for v in t]), device=dev)
    la2, la3 = DLD.lowres_affine_2d(f[1:], t[1:]), DLD.lowres_affine(f, t)

    def lowres2d():
        x.copy_(xin)
        DLD.lowres_gather_2d(x[0], d2[0], t[1:], flip)
        DLD.channel_stats(d2, st[0], ws)
        DLD.bspline_prefilter(d2, 6)
        DLD.spatial_transform_data_2d(d2, x, la2, flip, 0.0)
        DLD.intensity_apply(x, DLD.OP_CLIP, None, st[0])

    def lowres3d():
        x.copy_(xin)
        DLD.lowres_gather(x[0], d3[0], t, flip)
        DLD.channel_stats(d3, st[0], ws)
        DLD.bspline_prefilter(d3, 7)
        DLD.spatial_transform_data(d3, x, la3, flip, 0.0)
        DLD.intensity_apply(x, DLD.OP_CLIP, None, st[0])

    lowres2d()
    r2 = x.clone()
    lowres3d()
    print(f"dummy 2-D, low-res channel {f[0]}x{f[1]}x{f[2]} at zoom 0.75 (t = {t}): max |2-D - 3-D| = "
          f"{float((r2 - x).abs().max()):.2e}")
    td, te = _event_ms([lowres2d, lowres3d])
    md, _ = _row("dedicated (gather2d + prefilter 6 + warp2d)", td)
    me, se = _row("embedded 3-D (gather t[0]=D + prefilter 7 + warp)", te)
    print(f"  dedicated / embedded = {md / me:.3f} (allowed: 1 + max(3 %, baseline spread {se * 100:.1f} %))")

    # whole batches of the loader, reference probabilities
    ds = _DS(4, (80, 340, 340), channels=C)
    rot = {'x': (-np.pi, np.pi), 'y': (0, 0), 'z': (0, 0)}
    scales = [[1, 1, 1], [1, 0.5, 0.5], [0.5, 0.25, 0.25], [0.25, 0.125, 0.125]]
    for intensity in (False, True):
        dl = DeviceDataLoader3D(ds, 2, n, f, _L(), oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2),
                                deep_supervision_scales=scales, device="cuda:0", rotation_for_DA=rot,
                                do_dummy_2d_data_aug=True, intensity_augmentation=intensity)
        np.random.seed(0)
        for _ in range(4):
            next(dl)
        plans = [dl.plan_batch() for _ in range(60)]
        for p in plans[:10]:
            dl.generate_train_batch(p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in plans:
            dl.generate_train_batch(p)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / len(plans) * 1e3
        nmod = sum(s is not None for p in plans for s in p[2])
        print(f"dummy 2-D loader, batch 2, intensity {'on' if intensity else 'off'}: {ms:.3f} ms per batch "
              f"({nmod} of {2 * len(plans)} samples modified)")


if __name__ == "__main__":
    if "--dummy2d" in sys.argv:
        dummy2d()
    else:
        main()
