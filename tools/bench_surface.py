"""Times the surface metrics (HD, HD95, ASSD) of one case on the GPU box:
   python tools/bench_surface.py [--shape 288 384 384] [--labels 4] [--fills 0.01 0.1 0.5] [--iters 20] [--cpu]
Label volumes: per label a smooth random field, a voxel takes the label of the largest field where that exceeds a
threshold chosen so that about `fill` of the volume is foreground; the prediction is the ground truth rolled by
(2, -3, 1).  Per fill, at unit and at anisotropic spacing (2.5, 0.7, 0.7): the time of
evaluation.compute_surface_metrics per case (3 warm-up calls, host clock around a device synchronise), the bounding
boxes, and the bytes the passes must move (border pass: 2 label bytes read + 1 written per voxel and label; each of
the three transform passes, twice per label: the box read and written once in int32 or fp64, 1 byte read in pass W)
with the share of the 8 TB/s HBM peak that makes.  --cpu adds the scipy restatement (tests/surface_ref.py) on one host
core on the same inputs.  Kernel times: run under rocprofv3 --kernel-trace --stats in a run of its own.  Run
tools/bench_infer.py --no-mirror in the same session for the sliding-window time the metrics are compared with."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multimodal_mvd_seg_amd import evaluation, surface  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


def make_case(shape, nlabels, fill, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    coarse = torch.randn((1, nlabels, shape[0] // 24 + 2, shape[1] // 24 + 2, shape[2] // 24 + 2), generator=g)
    f = torch.nn.functional.interpolate(coarse.to(dev), size=tuple(shape), mode="trilinear")[0]
    top, arg = f.max(0)
    thr = torch.quantile(top.flatten()[::97].float(), 1.0 - fill)
    gt = torch.where(top > thr, arg + 1, torch.zeros_like(arg)).to(torch.uint8).contiguous()
    pred = torch.roll(gt, (2, -3, 1), (0, 1, 2)).contiguous()
    return gt, pred


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[288, 384, 384])
    ap.add_argument("--labels", type=int, default=4)
    ap.add_argument("--fills", type=float, nargs="+", default=[0.01, 0.1, 0.5])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface needs an MI355X")
    dev = torch.device("cuda:0")
    labels = list(range(1, args.labels + 1))
    nvox = args.shape[0] * args.shape[1] * args.shape[2]
    for fill in args.fills:
        gt, pred = make_case(args.shape, args.labels, fill, dev)
        boxes = []
        for l in labels:
            _, st = surface._border(pred, gt, [l], 1)
            boxes.append(surface._Stats(st.cpu().numpy(), gt.shape))
        boxvox = sum(b.box[3] * b.box[4] * b.box[5] for b in boxes)
        nborder = sum(b.nb_a + b.nb_b for b in boxes)
        print(f"fill {fill}: foreground {float((gt != 0).float().mean()):.3f} of {tuple(args.shape)}, boxes "
              f"{[tuple(b.box[3:]) for b in boxes]} = {boxvox / nvox / len(labels):.2f} of the volume per label, "
              f"{nborder} border voxels")
        for spacing, width in ((None, 4), ((2.5, 0.7, 0.7), 8)):
            t = timed(lambda: evaluation.compute_surface_metrics(gt, pred, labels, spacing=spacing), args.iters)
            b_border = len(labels) * 3 * nvox
            b_edt = 2 * boxvox * (1 + width + 2 * 2 * width)
            res = evaluation.compute_surface_metrics(gt, pred, labels, spacing=spacing)
            print(f"  spacing {spacing}: {t * 1e3:.2f} ms per case ({len(labels)} labels); compulsory traffic border pass "
                  f"{b_border / 1e6:.0f} MB + transforms {b_edt / 1e6:.0f} MB = {(b_border + b_edt) / t / HBM_PEAK * 100:.2f} % "
                  f"of HBM peak; label 1: {res[1]}")
            t = timed(lambda: [surface._border(pred, gt, [l], 1) for l in labels], args.iters)
            print(f"    border passes alone: {t * 1e3:.3f} ms, {b_border / t / HBM_PEAK * 100:.1f} % of HBM peak")
            if args.cpu:
                import surface_ref
                g, p = gt.cpu().numpy(), pred.cpu().numpy()
                t0 = time.perf_counter()
                ref = surface_ref.surface_metrics(g, p, labels[:1], spacing, 1)
                print(f"    scipy restatement, label 1 only, one core: {time.perf_counter() - t0:.1f} s "
                      f"(HD, HD95 and ASSD each transform twice); {ref[1]}")


if __name__ == "__main__":
    main()
