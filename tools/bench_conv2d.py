"""Micro-benchmark (GPU box) of the 9-tap in-plane (1x3x3) conv layers and of a 2-D train step:
   python tools/bench_conv2d.py [--launches 30] [--skip-step | --skip-layers | --small]
1. k_fwd_wino2p against the direct engine (the path of the same call with mvd_set_wino2p_min_items(1 << 40)), forward and
   input gradient;  2. the generic weight gradient at the same shapes (there is no Winograd one for 9 taps);  3. a 2-D train
   step in samples/s (batch 12, 512 x 512, 8 stages 32..512), fp32 eager and graphed, engine on and off.
HIP events per launch, warm-up, the two engines alternating launch by launch in one process, median of >= 20 launches."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_mvd_seg_amd import ops  # noqa: E402
from multimodal_mvd_seg_amd._lib import CONV_WINO2P, call, i3, query  # noqa: E402

# name: (N, C1, C2, K, D, H, W)
LAYERS = {
    "32->32 @ 12x512x512": (12, 32, 0, 32, 1, 512, 512),
    "64->64 @ 12x256x256": (12, 64, 0, 64, 1, 256, 256),
    "64+64->64 @ 12x256x256": (12, 64, 64, 64, 1, 256, 256),
    "32->32 @ 2x40x192x160 (anisotropic 3-D)": (2, 32, 0, 32, 40, 192, 160),
}
# --small: the deeper stages of the 2-D step network, down to the default work-item threshold (where it comes from)
SMALL = {
    "128->128 @ 12x128x128 (6144 items)": (12, 128, 0, 128, 1, 128, 128),
    "256->256 @ 12x64x64 (3072 items)": (12, 256, 0, 256, 1, 64, 64),
    "512->512 @ 12x32x32 (1536 items)": (12, 512, 0, 512, 1, 32, 32),
    "512->512 @ 12x16x16 (384 items)": (12, 512, 0, 512, 1, 16, 16),
    "512->512 @ 12x8x8 (96 items)": (12, 512, 0, 512, 1, 8, 8),
    "32->32 @ 3x40x56 (70 items)": (3, 32, 0, 32, 1, 40, 56),
}
DEV = torch.device("cuda:0")
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def alternate(fns, launches, warmup=5, reps=1):
    """fns: {name: (select, launch)}; every round times each once, in turn -> {name: median ms per launch}.  `select`
    (the engine switch, host only) runs outside the event pair; reps > 1 puts that many back-to-back launches into one
    pair, for layers of a few microseconds whose single launch is mostly launch and event overhead."""
    def group(f):
        for _ in range(reps):
            f()
    for _ in range(warmup):
        for sel, f in fns.values():
            sel()
            group(f)
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(launches):
        for k, (sel, f) in fns.items():
            sel()
            ev[k].append(timed(lambda: group(f)))
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in v) / reps for k, v in ev.items()}


def bench_layers(launches, layers=LAYERS, reps=1):
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ks, st = i3((1, 3, 3)), i3((1, 1, 1))
    for name, (N, C1, C2, K, D, H, W) in layers.items():
        C = C1 + C2
        x1 = ops.empty_cl3d((N, C1, D, H, W), DEV).normal_()
        x2 = ops.empty_cl3d((N, C2, D, H, W), DEV).normal_() if C2 else None
        w = torch.randn(K, C, 1, 3, 3, device=DEV) * 0.05
        wf, wb = ops.pack_weight(w, False)
        n = query("mvd_wino2p_weight_elems", C, K)
        pf, pb = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        call("mvd_pack_weight_wino2p", P(w), P(pf), P(pb), K, C, s)
        bias = torch.zeros(K, device=DEV)
        y = ops.empty_cl3d((N, K, D, H, W), DEV)
        dy = ops.empty_cl3d((N, K, D, H, W), DEV).normal_()
        dx1 = ops.empty_cl3d((N, C1, D, H, W), DEV)
        dx2 = ops.empty_cl3d((N, C2, D, H, W), DEV) if C2 else None
        dw, db = torch.empty_like(w), torch.empty(K, device=DEV)
        nb = max(query("mvd_conv3d_wgrad_workspace_bytes", C, K, 9, N, D, H, W),
                 query("mvd_conv_fwd_workspace_bytes", N, D * H * W, max(K, C)))
        ws = torch.empty(max(nb, 1024), dtype=torch.uint8, device=DEV)

        def select(on):
            return lambda: call("mvd_set_wino2p_min_items", 1 if on else 1 << 40)

        def fwd(on):
            return select(on), lambda: call("mvd_conv3d_fwd_routed", P(x1), C1, P(x2), C2, P(wf), P(pf), CONV_WINO2P, P(bias), P(y),
                                            None, 0, None, N, D, H, W, K, ks, st, P(ws), ws.numel(), s)

        def dgrad(on):
            return select(on), lambda: call("mvd_conv3d_dgrad_routed", P(dy), P(wb), P(pb), CONV_WINO2P, P(dx1), C1, P(dx2), C2, N,
                                            D, H, W, K, ks, st, P(ws), ws.numel(), s)

        def wgrad():
            call("mvd_conv3d_wgrad", P(x1), C1, P(x2), C2, P(dy), P(dw), P(db), N, D, H, W, K, ks, st, P(ws), ws.numel(), s)

        try:
            flops = 2.0 * 9 * C * K * N * D * H * W
            for what, mk in (("fwd", fwd), ("dgrad", dgrad)):
                r = alternate({"wino2p": mk(True), "direct": mk(False)}, launches, reps=reps)
                print(f"{name:42s} {what:5s}: wino2p {r['wino2p']:7.3f} ms  direct {r['direct']:7.3f} ms  "
                      f"ratio {r['direct'] / r['wino2p']:5.2f}x  ({flops / r['wino2p'] / 1e9:6.1f} direct-equivalent TFLOP/s)",
                      flush=True)
            r = alternate({"wgrad": (lambda: None, wgrad)}, launches, reps=reps)
            print(f"{name:42s} wgrad: generic {r['wgrad']:7.3f} ms  ({flops / r['wgrad'] / 1e9:6.1f} TFLOP/s)", flush=True)
        finally:
            call("mvd_set_wino2p_min_items", -1)
        del x1, x2, y, dy, dx1, dx2, ws


def bench_step(launches):
    from multimodal_mvd_seg_amd import trainer
    strides = [[1, 1]] + [[2, 2]] * 7
    plans = trainer.make_plans((512, 512), strides, batch_size=12, base_features=32, max_features=512, configuration='2d')
    ds = {"channel_names": {"0": "a"}, "labels": {"background": 0, "a": 1, "b": 2}}
    for graph in (False, True):
        for on in (True, False):
            try:
                call("mvd_set_wino2p_min_items", -1 if on else 1 << 40)
                tr = trainer.nnUNetTrainerMI355(plans, "2d", 0, ds, device=DEV)
                tr.use_hip_graph = graph
                tr.initialize()
                tr.network.train()
                b = tr.make_dummy_batch()
                for _ in range(6):
                    tr.train_step(b, return_device_loss=True)
                torch.cuda.synchronize()
                ev = [timed(lambda: tr.train_step(b, return_device_loss=True)) for _ in range(launches)]
                torch.cuda.synchronize()
                ms = statistics.median(a.elapsed_time(c) for a, c in ev)
                print(f"2-D train step, batch 12, 512x512, 8 stages, fp32 {'graphed' if graph else 'eager  '}, 9-tap engine "
                      f"{'default' if on else 'off    '}: {ms:8.2f} ms/step  {12e3 / ms:7.1f} samples/s", flush=True)
                del tr, b
            finally:
                call("mvd_set_wino2p_min_items", -1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--small", action="store_true", help="the small-layer sweep behind the default threshold, alone")
    a = ap.parse_args()
    assert a.launches >= 20, "median of at least 20 launches"
    if a.small:
        bench_layers(a.launches, SMALL, reps=20)   # 20 back-to-back launches per event pair
        sys.exit(0)
    if not a.skip_layers:
        bench_layers(a.launches)
    if not a.skip_step:
        bench_step(a.launches)
