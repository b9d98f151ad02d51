"""Times the segmentation export and the confusion counts on the GPU box:
   python tools/bench_export.py [--logits 5 192 256 256] [--iters 20] [--cpu]
For the 1.5x-per-axis upsampling (192x256x256 -> 288x384x384) and for the equal-shape case, each with the identity and
with a permuting transpose_backward: time per volume of the export (argmax path; the softmax path beside it) and of the
counts, and the share of the HBM peak on the compulsory traffic (K*d*h*w*4 bytes read once + D*H*W bytes written; 2 bytes
per voxel read for the counts).  --cpu adds the same export by the scipy oracle (fp64 zoom per channel, fp32 softmax,
argmax) on one thread and with the channels spread over up to 16 threads.  Run tools/bench_infer.py --no-mirror in the
same session for the sliding-window time the export is compared with."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_mvd_seg_amd import evaluation, export  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


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
    ap.add_argument("--logits", type=int, nargs=4, default=[5, 192, 256, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_export needs an MI355X")
    dev = torch.device("cuda:0")
    K, d, h, w = args.logits
    g = torch.Generator(device="cpu").manual_seed(0)
    coarse = torch.randn((1, K, d // 4 + 1, h // 4 + 1, w // 4 + 1), generator=g) * 8
    x = torch.nn.functional.interpolate(coarse, size=(d, h, w), mode="trilinear")[0].contiguous().to(dev)
    up = (d * 3 // 2, h * 3 // 2, w * 3 // 2)
    total_ms = {}
    for name, new in (("1.5x", up), ("equal", (d, h, w))):
        nvox = new[0] * new[1] * new[2]
        comp = K * d * h * w * 4 + nvox
        for tb in ((0, 1, 2), (2, 0, 1)):
            t = timed(lambda: export.resize_logits_to_segmentation(x, new, new, (0, 0, 0), tb), args.iters)
            print(f"export {name} {(d, h, w)} -> {new} transpose_backward {tb}: {t * 1e3:.3f} ms/volume, "
                  f"{nvox / t / 1e9:.2f} Gvoxel/s, {comp / t / HBM_PEAK * 100:.1f} % of HBM peak on {comp / 1e6:.0f} MB")
            total_ms[(name, tb)] = t * 1e3
        t = timed(lambda: export.resize_logits_to_segmentation(x, new, new, (0, 0, 0), (0, 1, 2), None, True),
                  max(2, args.iters // 4))
        print(f"export {name} with probabilities (argmax + softmax kernels): {t * 1e3:.3f} ms/volume")
        seg = export.resize_logits_to_segmentation(x, new, new, (0, 0, 0))
        gt = torch.roll(seg, 3, 2).to(torch.int16)
        labels = list(range(1, K))
        for ref, what in ((gt, "int16"), (gt.to(torch.uint8), "uint8")):
            t = timed(lambda: evaluation.confusion_counts(ref, seg, labels), args.iters)
            b = nvox * (1 + ref.element_size())
            print(f"counts {name} {new} gt {what}, {len(labels)} labels: {t * 1e3:.3f} ms/volume, "
                  f"{b / t / HBM_PEAK * 100:.1f} % of HBM peak on {b / 1e6:.0f} MB")
            total_ms[(name, what)] = t * 1e3
        print(f"export + counts {name} (identity order, int16 gt): "
              f"{total_ms[(name, (0, 1, 2))] + total_ms[(name, 'int16')]:.3f} ms")
    if args.cpu:
        import scipy.ndimage as ndi
        xs = x.cpu().numpy()

        def one(c):
            return ndi.zoom(c.astype(np.float64), [o / i for o, i in zip(up, c.shape)], order=1, mode='nearest',
                            grid_mode=True)

        def tail(res):
            return torch.softmax(torch.from_numpy(np.stack(res).astype(np.float32)), 0).argmax(0).numpy().astype(np.uint8)

        torch.set_num_threads(1)
        t0 = time.perf_counter()
        ref = tail([one(c) for c in xs])
        t1 = time.perf_counter() - t0
        torch.set_num_threads(16)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            ref16 = tail(list(pool.map(one, xs)))
        t16 = time.perf_counter() - t0
        seg = export.resize_logits_to_segmentation(x, up, up, (0, 0, 0)).cpu().numpy()
        print(f"scipy oracle 1.5x: {t1:.2f} s on one thread, {t16:.2f} s with {K} channels over up to 16 threads; "
              f"labels differing from the device: {float((seg != ref).mean()):.2e} of the voxels "
              f"(threads identical: {np.array_equal(ref, ref16)})")


if __name__ == "__main__":
    main()
