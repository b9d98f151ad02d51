"""Per-layer time of the fp32 weight gradient (mvd_conv3d_wgrad, bias included) of the stride-1 3x3x3 layers of configs[1]
(batch 2, NDHWC) with k_wgrad_wino3 forced on and off (mvd_set_wgrad_wino3_min_items); CUDA events, median of the last
5 of 8 calls.  Prints one line per layer and the ratio 3-D / 2-D."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_mvd_seg_amd import _lib  # noqa: E402

LAYERS = [(128, 32, 0, 32), (128, 32, 32, 32), (64, 64, 0, 64), (64, 64, 64, 64), (32, 128, 0, 128),
          (32, 128, 128, 128), (16, 256, 0, 256), (16, 256, 256, 256)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def time_layer(S, C1, C2, K, on, N=2):
    dev = torch.device("cuda:0")
    x1 = torch.randn(N, S, S, S, C1, device=dev)
    x2 = torch.randn(N, S, S, S, C2, device=dev) if C2 else None
    dy = torch.randn(N, S, S, S, K, device=dev)
    nbytes = _lib.query("mvd_conv3d_wgrad_workspace_bytes", C1 + C2, K, 27, N, S, S, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dw = torch.empty(K, C1 + C2, 27, device=dev)
    db = torch.empty(K, device=dev)
    _lib.call("mvd_set_wgrad_wino3_min_items", 1 if on else 1 << 40)
    try:
        ts = []
        for _ in range(8):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.call("mvd_conv3d_wgrad", _p(x1), C1, _p(x2), C2, _p(dy), _p(dw), _p(db), N, S, S, S, K,
                      _lib.i3((3, 3, 3)), _lib.i3((1, 1, 1)), _p(ws), ctypes.c_size_t(nbytes),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts[3:])[2]
    finally:
        _lib.call("mvd_set_wgrad_wino3_min_items", -1)


def main():
    _lib.load()
    print(" S    C1+C2 -> K     F(2x2,3x3) ms   F(2x2x2,3x3x3) ms   ratio   default")
    for S, C1, C2, K in LAYERS:
        t2 = time_layer(S, C1, C2, K, False)
        t3 = time_layer(S, C1, C2, K, True)
        dflt = _lib.query("mvd_conv_wgrad_wino3_applicable", 2, S, S, S, C1, C2, K, _lib.i3((3, 3, 3)), _lib.i3((1, 1, 1)))
        ch = f"{C1}+{C2}" if C2 else f"{C1}"
        print(f"{S:4d}  {ch:>8s} -> {K:<4d}  {t2:10.3f}      {t3:10.3f}        {t3 / t2:6.3f}   {'3-D' if dflt else '2-D'}")


if __name__ == "__main__":
    main()
