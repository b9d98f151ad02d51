"""Times one forward + backward of the 3-D cubical persistence loss (losses.CubicalWassersteinLoss, dimension 2, q = 2) at
2 x 64 x 128 x 256 -- the vessel logit channel of the dual-branch trainer's patch -- on a smooth field (Gaussian-filtered
noise with planted blobs) and on white noise (the worst case: the most bars), split into keys + sort, the D2H copy, the
host pairing sweep, the H2D copy of the bars, target count + matching + loss, and the backward.  For scale it also times the
soft-clDice term (the default topo_term) at the same shape.

    python tools/bench_cubical_topo.py [--steps 5] [--warmup 2] [--dim 2]

Run by hand on the MI355X; prints one JSON line per field.  No target time is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (2, 64, 128, 256)


def smooth_field(seed=1):
    """logit-like: Gaussian-filtered noise (sigma 4 voxels) scaled to about [-4, 4], with planted closed shells"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    f = np.stack([ndimage.gaussian_filter(rng.standard_normal(SHAPE[1:]), 4.0) for _ in range(SHAPE[0])])
    f = (f / np.abs(f).max() * 4.0).astype(np.float32)
    mask = np.zeros(SHAPE, np.float32)
    for n in range(SHAPE[0]):
        for _ in range(24):
            c = [int(rng.integers(8, s - 8)) for s in SHAPE[1:]]
            r = int(rng.integers(2, 5))
            sl = tuple(slice(ci - r, ci + r + 1) for ci in c)
            f[n][sl] += 3.0
            mask[n][sl] = 1
    return f, mask


def white_noise(seed=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(SHAPE).astype(np.float32), (rng.random(SHAPE) < 0.2).astype(np.float32)


def median(rows, key):
    return float(np.median([r[key] for r in rows]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dim", type=int, default=2)
    a = ap.parse_args()
    from multimodal_mvd_seg_amd import losses, ops
    dev = torch.device("cuda:0")
    for name, (f, mask) in (("smooth", smooth_field()), ("white_noise", white_noise())):
        x0, t = torch.from_numpy(f).to(dev), torch.from_numpy(mask).to(dev)
        layer = losses.CubicalWassersteinLoss(a.dim, 2)
        rows = []
        for it in range(a.warmup + a.steps):
            x = x0.clone().requires_grad_(True)
            ops.Cub3dTimes.on = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            l = layer(x, t)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            l.backward()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ops.Cub3dTimes.on = False
            r = dict(ops.Cub3dTimes.last)
            r["forward_ms"], r["backward_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            r["target_count_ms"] = r["forward_ms"] - sum(r[k] for k in ("keys_sort_ms", "d2h_ms", "host_sweep_ms", "h2d_ms",
                                                                         "match_loss_ms"))
            if it >= a.warmup:
                rows.append(r)
        out = {"field": name, "shape": list(SHAPE), "dim": a.dim, "q": 2, "loss": float(l.detach()), "bars": rows[-1]["bars"],
               "m": layer.last_m.tolist()}
        for k in ("keys_sort_ms", "d2h_ms", "host_sweep_ms", "h2d_ms", "target_count_ms", "match_loss_ms", "forward_ms",
                  "backward_ms"):
            out[k] = round(median(rows, k), 3)
        print(json.dumps(out), flush=True)
    # the soft-clDice term at the same shape, forward + backward, for scale
    prob = torch.sigmoid(torch.from_numpy(smooth_field()[0]).to(dev))[:, None].contiguous()
    tm = torch.from_numpy(smooth_field()[1]).to(dev)[:, None].contiguous()
    ts = []
    for it in range(a.warmup + a.steps):
        p = prob.clone().requires_grad_(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses.soft_cldice(p, tm, 3).backward()
        torch.cuda.synchronize()
        if it >= a.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"field": "soft_cldice(iter 3) fwd+bwd", "shape": list(SHAPE), "ms": round(float(np.median(ts)), 3)}), flush=True)


if __name__ == "__main__":
    main()
