"""Time of the fp32 InstanceNorm + LeakyReLU entry points (mvd_instnorm_lrelu_fwd / _bwd) per layer shape of the deep stages
of configs[1] (batch 2, NDHWC) in the three-launch form and the single-launch form (mvd_set_instnorm_small_max).  The step
runs as a hipGraph, so each form is timed the same way: REPS back-to-back calls captured into one graph, CUDA events around a
replay, median of 7 replays, per call.  Prints one line per shape and direction; '-' where the rows of a sample do not fit
the single launch's registers (mvd_instnorm_single_launch)."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_mvd_seg_amd import _lib  # noqa: E402

# (spatial, channels): the 32^3 .. 4^3 stages of configs[1] and two sizes between 16^3 and 8^3 that bracket the limit
SHAPES = [((32, 32, 32), 128), ((16, 16, 16), 256), ((8, 16, 16), 256), ((8, 8, 16), 320), ((8, 8, 8), 320), ((4, 4, 4), 320)]
REPS = 20


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def time_shape(S, C, backward, small, N=2):
    dev = torch.device("cuda:0")
    V = S[0] * S[1] * S[2]
    x, dy = torch.randn(N, V, C, device=dev), torch.randn(N, V, C, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    mean, rstd = torch.empty(N, C, device=dev), torch.empty(N, C, device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    nbytes = _lib.query("mvd_instnorm_workspace_bytes", N, V, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("mvd_set_instnorm_small_max", (1 << 40) if small else 0)
    try:
        if small and not _lib.query("mvd_instnorm_single_launch", V, C):
            return None

        def run():
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if backward:
                _lib.call("mvd_instnorm_lrelu_bwd", _p(x), _p(dy), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db),
                          N, V, C, 0.01, _p(ws), ctypes.c_size_t(nbytes), st)
            else:
                _lib.call("mvd_instnorm_lrelu_fwd", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), N, V, C, 1e-5, 0.01,
                          _p(ws), ctypes.c_size_t(nbytes), st)
        _lib.call("mvd_instnorm_lrelu_fwd", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), N, V, C, 1e-5, 0.01, _p(ws),
                  ctypes.c_size_t(nbytes), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            run()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(REPS):
                    run()
        ts = []
        for _ in range(9):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / REPS)
        return sorted(ts[2:])[len(ts[2:]) // 2]
    finally:
        _lib.call("mvd_set_instnorm_small_max", -1)


def main():
    print(f"{'shape (N=2)':>16} {'V x C':>9} {'dir':>4} {'3 launches us':>14} {'1 launch us':>12}")
    for S, C in SHAPES:
        for backward in (False, True):
            t3, t1 = time_shape(S, C, backward, False), time_shape(S, C, backward, True)
            print(f"{'%dx%dx%d x %d' % (*S, C):>16} {S[0] * S[1] * S[2] * C:>9} {'bwd' if backward else 'fwd':>4} {t3:>14.2f} "
                  f"{('%12.2f' % t1) if t1 is not None else '           -'}", flush=True)


if __name__ == "__main__":
    main()
