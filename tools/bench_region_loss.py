"""Kernel rate of the region loss: forward + finalize + backward of mvd_dcbce_* at [2, 3, 128^3] in the label-map
form (with and without the ignore bit) and in the plane form, next to mvd_dcce_* at [2, 4, 128^3] -- optionally from another
build of the library (--baseline-lib: e.g. the parent commit's), alternated with it in the same session.

usage: python tools/bench_region_loss.py [--baseline-lib PATH] [--reps 5] [--iters 20]
Prints one JSON line per variant: ms per fwd+finalize+bwd (median of the repetitions and their min / max), the compulsory
bytes (logits read twice, targets read twice, gradient written once) and the share of 8 TB/s."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_mvd_seg_amd import _lib, ops  # noqa: E402

PEAK = 8e12


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    base = lib
    if a.baseline_lib:
        base = ctypes.CDLL(a.baseline_lib)
        for name in ("mvd_dcce_workspace_bytes", "mvd_dcce_fwd", "mvd_dcce_finalize", "mvd_dcce_bwd"):
            getattr(base, name).restype, getattr(base, name).argtypes = _lib.SIGNATURES[name]
    N, S = 2, a.size
    V = S ** 3
    g = torch.Generator().manual_seed(0)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    one = torch.ones(1, device=dev)
    regions = [(1, 2, 3), (2, 3), 3]

    def region_variant(R, form, ignore):
        z = (torch.randn((N, R, V), generator=g) * 3).to(dev)
        seg = torch.randint(0, 5 if ignore else 4, (N, 1, V), generator=g).float().to(dev)
        lut = ops.region_label_table(regions, 4 if ignore else None)
        t = seg if form == 0 else ops.convert_seg_to_regions(seg, regions, 4 if ignore else None).contiguous()
        lp = lut.ctypes.data_as(ctypes.c_void_p) if form == 0 else None
        stats = torch.empty((N, 3 * R + 2), device=dev)
        ws = torch.empty(lib.mvd_dcbce_workspace_bytes(N, V, R), dtype=torch.uint8, device=dev)
        loss, coef, dl = torch.empty(4, device=dev), torch.empty((N, R, 2), device=dev), torch.empty_like(z)

        def run():
            rc = lib.mvd_dcbce_fwd(p(z), p(t), form, lp, p(stats), N, V, R, p(ws), ws.numel(), st())
            rc |= lib.mvd_dcbce_finalize(p(stats), N, p(stats), N, p(loss), p(coef), V, R, 1, 1, int(ignore), 1e-5, 1.0, 1.0, st())
            rc |= lib.mvd_dcbce_bwd(p(z), p(t), form, lp, p(coef), p(loss), p(one), 1.0, p(dl), N, V, R, 1.0, st())
            assert rc == 0, lib.mvd_last_error()
        planes = 1 if form == 0 else R + int(ignore)
        return run, 4 * N * V * (2 * R + 2 * planes + R)

    def softmax_variant(l, K):
        z = (torch.randn((N, K, V), generator=g) * 3).to(dev)
        t = torch.randint(0, K, (N, V), generator=g).float().to(dev)
        stats = torch.empty((N, 3 * K + 1), device=dev)
        ws = torch.empty(l.mvd_dcce_workspace_bytes(N, V, K), dtype=torch.uint8, device=dev)
        loss, coef, dl = torch.empty(3, device=dev), torch.empty((N, K, 2), device=dev), torch.empty_like(z)

        def run():
            rc = l.mvd_dcce_fwd(p(z), p(t), p(stats), N, V, K, p(ws), ws.numel(), st())
            rc |= l.mvd_dcce_finalize(p(stats), N, p(stats), N, p(loss), p(coef), V, K, 1, 0, 1e-5, 1.0, 1.0, st())
            rc |= l.mvd_dcce_bwd(p(z), p(t), p(coef), p(one), 1.0, p(dl), N, V, K, 1.0, st())
            assert rc == 0
        return run, 4 * N * V * (2 * K + 2 + K)

    variants = {
        "dcbce label map [2,3,%d^3]" % S: region_variant(3, 0, False),
        "dcbce label map + ignore [2,3,%d^3]" % S: region_variant(3, 0, True),
        "dcbce planes [2,3,%d^3]" % S: region_variant(3, 1, False),
        "dcbce planes + ignore [2,3,%d^3]" % S: region_variant(3, 2, True),
        ("dcce baseline lib [2,4,%d^3]" if a.baseline_lib else "dcce [2,4,%d^3]") % S: softmax_variant(base, 4),
    }
    times = {k: [] for k in variants}
    for run, _ in variants.values():
        for _ in range(5):
            run()
    torch.cuda.synchronize()
    for _ in range(a.reps):       # alternate the variants inside every repetition
        for name, (run, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    for name, (_, nbytes) in variants.items():
        ms = float(np.median(times[name]))
        print(json.dumps({"variant": name, "ms": round(ms, 5), "ms_min": round(min(times[name]), 5),
                          "ms_max": round(max(times[name]), 5), "bytes": nbytes, "TB_per_s": round(nbytes / ms / 1e9, 3),
                          "share_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 3)}))


if __name__ == "__main__":
    main()
