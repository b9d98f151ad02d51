"""Ensemble export and fold prediction on one MI355X.

Ensemble export, K = 5, M in {2, 5} members of 192x256x256 logits to a 288x384x384 segmentation, three ways:
  (a) parent   the way open before the ensembling module: export.resize_logits_to_segmentation(return_probabilities=True)
               per member, then torch.stack(probs).mean(0).argmax(0)
  (b) chain    the unfused device chain: the same per-member export, then ensembling.merge_probabilities
               (mvd_ensemble_mean_argmax)
  (c) fused    ensembling.ensemble_logits_to_segmentation: one launch of mvd_export_ensemble_argmax_u8
(b) and (c) give the same labels bit for bit (checked here before timing); (a) is compared and its differing voxels
counted (torch's mean sums in another order).  GB/s is the COMPULSORY traffic -- every member's logits read once plus one
byte per output voxel -- over the time: the same numerator for all three, so that it ranks them.

Fold prediction, M = 5 parameter sets of a small PlainConvUNet on a 2 x 96x128x128 case (patch 64^3, no mirroring):
SlidingWindowPredictor.predict_logits_from_preprocessed_data against load_state_dict + predict_sliding_window_return_logits
per fold with torch `+=` and `/= 5`; and the fold loop's tail alone at [5, 192x256x256]: mvd_sw_normalize_add against
mvd_sw_normalize + torch add (+ divide on the last fold).

usage: python tools/bench_ensemble.py [--reps 21] [--fold-reps 5] [--out FILE]
Times are device events around one call, warmed up, variants alternated inside every repetition; median, min and max of the
repetitions.  Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_mvd_seg_amd import _lib, ensembling, export, trainer  # noqa: E402
from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor  # noqa: E402

DEV = torch.device("cuda:0")


def timed(variants, reps, warmup=3):
    """variants: {name: callable}; -> {name: [ms per repetition]}, the variants alternated inside every repetition"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times


def row(what, name, ts, **more):
    r = {"what": what, "variant": name, "ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4),
         "ms_max": round(max(ts), 4), "reps": len(ts)}
    r.update(more)
    return r


def bench_export(M, reps, K=5, shape=(192, 256, 256), new=(288, 384, 384)):
    g = torch.Generator(device=DEV).manual_seed(M)
    xs = [torch.randn((K, *shape), generator=g, device=DEV) * 2 for _ in range(M)]
    axes = [None] * M
    geom = (new, new, (0, 0, 0), (0, 1, 2))

    def parent():
        probs = [export.resize_logits_to_segmentation(x, *geom, None, return_probabilities=True)[1] for x in xs]
        return torch.stack(probs).mean(0).argmax(0)

    def chain():
        probs = [export.resize_logits_to_segmentation(x, *geom, None, return_probabilities=True)[1] for x in xs]
        return ensembling.merge_probabilities(probs, None)

    def fused():
        return ensembling.ensemble_logits_to_segmentation(xs, *geom, axes)

    a, b, c = parent(), chain(), fused()
    assert torch.equal(b, c), "the fused kernel and the unfused chain disagree"
    differ = int((a.to(torch.uint8) != c).sum())
    del a, b, c
    times = timed({"a parent": parent, "b chain": chain, "c fused": fused}, reps)
    nvox = int(np.prod(new))
    nbytes = 4 * K * M * int(np.prod(shape)) + nvox
    return [row(f"ensemble export K={K} M={M} {shape}->{new}", name, ts, compulsory_bytes=nbytes,
                GB_per_s=round(nbytes / np.median(ts) / 1e6, 1), voxels_parent_differs=differ)
            for name, ts in times.items()]


def bench_tail(reps, K=5, shape=(192, 256, 256), M=5):
    V = int(np.prod(shape))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    acc = torch.rand((K, V), device=DEV) + 1
    npred = torch.rand((V,), device=DEV) + 1
    total = torch.zeros((K, V), device=DEV)
    rows = []
    for label, first, last in (("middle fold", 0, 0), ("last fold", 0, 1)):
        def fused():
            _lib.call("mvd_sw_normalize_add", P(total), P(acc), P(npred), K, V, first, last, M, s())

        def separate():
            _lib.call("mvd_sw_normalize", P(acc), P(npred), K, V, s())
            total.add_(acc)
            if last:
                total.div_(M)
        times = timed({"mvd_sw_normalize_add": fused, "mvd_sw_normalize + torch": separate}, reps)
        rows += [row(f"fold tail, {label}, [{K}, {shape}]", name, ts) for name, ts in times.items()]
    return rows


def bench_folds(reps, M=5):
    ds = {"channel_names": {"0": "a", "1": "b"}, "labels": {"background": 0, "a": 1, "b": 2, "c": 3, "d": 4}}
    plans = trainer.make_plans((64, 64, 64), [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2]], base_features=32,
                               max_features=256)
    pm = trainer.PlansManager(plans)
    cm = pm.get_configuration('3d_fullres')
    sds = []
    for i in range(M):
        torch.manual_seed(i)
        n = trainer.get_network_from_plans(pm, ds, cm, 2, deep_supervision=True)
        sds.append({k: v.detach().clone().to(DEV) for k, v in n.state_dict().items()})
    net = trainer.get_network_from_plans(pm, ds, cm, 2, deep_supervision=True).to(DEV)
    img = torch.randn((2, 96, 128, 128), device=DEV)
    kw = dict(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV)
    pred = SlidingWindowPredictor(net, (64, 64, 64), 5, list_of_parameters=sds, **kw)
    single = SlidingWindowPredictor(net, (64, 64, 64), 5, **kw)

    def folds():
        return pred.predict_logits_from_preprocessed_data(img)

    def singles():
        total = None
        for sd in sds:
            net.load_state_dict(sd)
            p = single.predict_sliding_window_return_logits(img)
            if total is None:
                total = p
            else:
                total += p
        total /= M
        return total

    assert torch.equal(folds(), singles()), "fold prediction and the per-fold loop disagree"
    times = timed({"predict_logits_from_preprocessed_data": folds, "5 single predictions + torch": singles}, reps,
                  warmup=1)
    return [row(f"fold prediction M={M}, case 2x96x128x128, patch 64^3, no mirroring", name, ts)
            for name, ts in times.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--fold-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py needs an MI355X: there is nothing to measure without one")
    _lib.load()
    rows = [{"device": torch.cuda.get_device_name(0), "reps": a.reps, "fold_reps": a.fold_reps}]
    for M in (2, 5):
        rows += bench_export(M, a.reps)
        torch.cuda.empty_cache()
    rows += bench_tail(a.reps)
    rows += bench_folds(a.fold_reps)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
