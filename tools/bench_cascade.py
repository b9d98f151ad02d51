"""Times the worst-case cascade stage of one batch of the device feed at the bench.py patch: 128^3, batch 2,
K = 3 one-hot channels; every channel takes a closing with a ball of r = 7.99 (16^3, 1736 voxels), then a component removal
on every channel.  HIP events after a warm-up, median of the rounds, beside the fp32 train step of bench.py's
configuration measured in the same process.

  python tools/bench_cascade.py            the device stage, its parts, and the train step
  python tools/bench_cascade.py --cpu      tests/cascade_ref.py (scipy.ndimage) on one host core: ONE closing and ONE
                                           removal at 128^3, to be multiplied by the 6 (sample, channel) pairs; no GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PATCH, B, K, RADIUS = (128, 128, 128), 2, 3, 7.99


def onehot_batch(seed=0):
    """[B, K, 128^3] bool: blobs of three labels from a smoothed random field, the look of a low-resolution prediction."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(seed)
    out = np.zeros((B, K, *PATCH), dtype=bool)
    for b in range(B):
        f = ndi.gaussian_filter(rng.standard_normal((K + 1, *PATCH)).astype(np.float32), (0, 6, 6, 6))
        lab = f.argmax(0)
        specks = rng.random(PATCH) < 2e-4     # plus small components for the removal to choose from
        lab[specks] = rng.integers(1, K + 1, int(specks.sum()))
        for k in range(K):
            out[b, k] = lab == k + 1
    return out


def cpu():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cascade_ref as REF
    planes = onehot_batch()[0]
    t0 = time.perf_counter()
    REF.apply_operator(planes, 0, 2, RADIUS)
    t1 = time.perf_counter()
    chan = planes[1].astype(np.float32)
    REF.remove_component(chan, u=0.5)
    t2 = time.perf_counter()
    print(f"cascade_ref on one host core, 128^3: closing r={RADIUS} + added-voxel rule {t1 - t0:.2f} s, removal "
          f"{t2 - t1:.2f} s; x {B * K} (sample, channel) pairs = {(t2 - t0) * B * K:.1f} s per worst-case batch")


def _median_ms(fn, warmup=3, rounds=15):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times)
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def main():
    import torch
    from multimodal_mvd_seg_amd import dataloading as DLD, trainer
    dev = torch.device("cuda:0")
    src = torch.from_numpy(onehot_batch().astype(np.float32)).to(dev)
    x = src.clone()
    bits = DLD.cascade_bitplanes(K, PATCH, dev)
    tmp = DLD.cascade_bitplanes(2, PATCH, dev)
    ws = DLD.cascade_remove_workspace(PATCH, dev)
    chosen = torch.zeros(2, dtype=torch.int32, device=dev)
    thr = DLD.cascade_removal_threshold(int(np.prod(PATCH)))
    rows = DLD.ball_rows(RADIUS)

    def pack_unpack():
        for b in range(B):
            DLD.cascade_pack(x[b], bits)
            DLD.cascade_unpack(bits, x[b])

    def morph():
        for b in range(B):
            for c in range(K):
                DLD.cascade_morph(bits, tmp, K, PATCH, c, 2, rows)

    def removal():
        for b in range(B):
            for c in range(K):
                DLD.cascade_remove(x[b, c], (c + 0.5) / K, thr, ws, chosen)

    def stage():
        x.copy_(src)
        for b in range(B):
            DLD.cascade_pack(x[b], bits)
            for c in range(K):
                DLD.cascade_morph(bits, tmp, K, PATCH, c, 2, rows)
            DLD.cascade_unpack(bits, x[b])
            for c in range(K):
                DLD.cascade_remove(x[b, c], (c + 0.5) / K, thr, ws, chosen)

    print(f"worst-case cascade stage, batch {B}, K = {K}, {PATCH[0]}^3, closing r = {RADIUS} ({len(rows)} table rows) + removal "
          f"on every channel; median (p10, p90) of 15 rounds, HIP events")
    res = {}
    for name, fn in (("pack + unpack (2 samples)", pack_unpack), ("6 closings + added-voxel rule", morph),
                     ("6 removals (label, sizes, pick, clear)", removal), ("whole stage (incl. reset copy)", stage)):
        res[name] = _median_ms(fn)
        print(f"  {name:<42s} {res[name][0]:9.3f} ms  ({res[name][1]:.3f}, {res[name][2]:.3f})")

    import bench
    plans = trainer.make_plans(PATCH, bench.STRIDES, batch_size=bench.PER_GPU_BATCH)
    tr = trainer.nnUNetTrainerMI355Benchmark_noDataLoading(plans, "3d_fullres", 0, bench.dataset_json(), device=dev)
    torch.manual_seed(0)
    tr.initialize()
    tr.on_train_epoch_start()
    for _ in range(8):
        tr.train_step(tr.dummy_batch, return_device_loss=True)
    step = _median_ms(lambda: tr.train_step(tr.dummy_batch, return_device_loss=True), warmup=2, rounds=15)
    print(f"  {'fp32 train step (bench.py configuration)':<42s} {step[0]:9.3f} ms  ({step[1]:.3f}, {step[2]:.3f})")
    whole = res["whole stage (incl. reset copy)"][0]
    print(f"  stage / step = {whole / step[0] * 100:.2f} %")


if __name__ == "__main__":
    cpu() if "--cpu" in sys.argv else main()
