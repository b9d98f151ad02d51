"""Time of the fused BatchNorm3d + LeakyReLU entry points (mvd_batchnorm_lrelu_fwd / _eval / _bwd) in fp32 and bf16 storage
at three layer shapes of the benchmark network, and in the same session of the InstanceNorm entry points at the same shapes
(mvd_instnorm_lrelu_fwd / _bwd and their _bf16 twins): InstanceNorm moves the same bytes and is the yardstick.

HIP events around REPS back-to-back calls after a warm-up, median of 7 rounds, per call; TB/s on the algorithmic bytes
(training forward 3, eval forward 2, backward 5 tensor passes of N * V * C elements).

--steps: additionally time full train steps of nnUNetTrainerBNMI355 and nnUNetTrainerMI355 at the bench.py workload
(4 x 128^3, batch 2) in fp32 and bf16: --warmup untimed steps, then --steps timed ones."""
import argparse
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_mvd_seg_amd import _lib  # noqa: E402

SHAPES = [(2, 32, (128, 128, 128)), (2, 64, (64, 64, 64)), (2, 320, (4, 4, 4))]
REPS = 10


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _time(run):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            run()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / REPS)
    return sorted(ts)[len(ts) // 2]


def time_shape(N, C, S, bf16):
    dev = torch.device("cuda:0")
    V = S[0] * S[1] * S[2]
    dt = torch.bfloat16 if bf16 else torch.float32
    x, dy = torch.randn(N, V, C, device=dev).to(dt), torch.randn(N, V, C, device=dev).to(dt)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    b = int(bf16)
    # BatchNorm
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    nb = _lib.query("mvd_batchnorm_workspace_bytes", N, V, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = {}
    out["bn fwd"] = _time(lambda: _lib.call("mvd_batchnorm_lrelu_fwd", _p(x), b, _p(gamma), _p(beta), _p(y), b, _p(mean), _p(rstd),
                                            _p(rm), _p(rv), _p(nbt), N, V, C, 1e-5, 0.1, 0.01, _p(ws), nb, _st()))
    out["bn eval"] = _time(lambda: _lib.call("mvd_batchnorm_lrelu_eval", _p(x), b, _p(gamma), _p(beta), _p(y), b, _p(rm), _p(rv),
                                             N, V, C, 1e-5, 0.01, _st()))
    out["bn bwd"] = _time(lambda: _lib.call("mvd_batchnorm_lrelu_bwd", _p(x), b, _p(dy), b, _p(gamma), _p(beta), _p(mean), _p(rstd),
                                            _p(dx), _p(dg), _p(db), N, V, C, 0.01, _p(ws), nb, _st()))
    # InstanceNorm, the yardstick
    imean, irstd = torch.empty(N, C, device=dev), torch.empty(N, C, device=dev)
    nbi = _lib.query("mvd_instnorm_workspace_bytes", N, V, C)
    wsi = torch.empty(nbi, dtype=torch.uint8, device=dev)
    if bf16:
        out["in fwd"] = _time(lambda: _lib.call("mvd_instnorm_lrelu_fwd_bf16", _p(x), 1, _p(gamma), _p(beta), _p(y), _p(imean),
                                                _p(irstd), N, V, C, 1e-5, 0.01, _p(wsi), nbi, _st()))
        out["in bwd"] = _time(lambda: _lib.call("mvd_instnorm_lrelu_bwd_bf16", _p(x), 1, _p(dy), _p(gamma), _p(beta), _p(imean),
                                                _p(irstd), _p(dx), _p(dg), _p(db), N, V, C, 0.01, _p(wsi), nbi, _st()))
    else:
        out["in fwd"] = _time(lambda: _lib.call("mvd_instnorm_lrelu_fwd", _p(x), _p(gamma), _p(beta), _p(y), _p(imean), _p(irstd),
                                                N, V, C, 1e-5, 0.01, _p(wsi), nbi, _st()))
        out["in bwd"] = _time(lambda: _lib.call("mvd_instnorm_lrelu_bwd", _p(x), _p(dy), _p(gamma), _p(beta), _p(imean), _p(irstd),
                                                _p(dx), _p(dg), _p(db), N, V, C, 0.01, _p(wsi), nbi, _st()))
    return out


PASSES = {"fwd": 3, "eval": 2, "bwd": 5}


def kernels():
    print(f"{'shape':>18} {'dtype':>5} {'call':>8} {'ms':>9} {'TB/s':>7}")
    for N, C, S in SHAPES:
        for bf16 in (False, True):
            elems = N * S[0] * S[1] * S[2] * C
            for name, ms in time_shape(N, C, S, bf16).items():
                nbytes = PASSES[name.split()[1]] * elems * (2 if bf16 else 4)
                print(f"{'[%d,%d,%d^3]' % (N, C, S[0]):>18} {'bf16' if bf16 else 'fp32':>5} {name:>8} {ms:>9.4f} "
                      f"{nbytes / (ms * 1e-3) / 1e12:>7.3f}", flush=True)


def steps(n_steps, warmup):
    import bench
    from multimodal_mvd_seg_amd import trainer
    dev = torch.device("cuda:0")
    print(f"{'trainer':>22} {'prec':>5} {'ms/step':>9} {'samples/s':>10}")
    for precision in ("fp32", "bf16"):
        for cls in (trainer.nnUNetTrainerMI355, trainer.nnUNetTrainerBNMI355):
            plans = trainer.make_plans(bench.PATCH, bench.STRIDES, batch_size=bench.PER_GPU_BATCH)
            t = cls(plans, "3d_fullres", 0, bench.dataset_json(), device=dev)
            torch.manual_seed(0)
            t.precision = precision
            t.initialize()
            batch = t.make_dummy_batch()
            t.on_train_epoch_start()
            t.hip_graph_warmup = min(t.hip_graph_warmup, max(1, warmup - 1))
            for _ in range(warmup):
                t.train_step(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                t.train_step(batch)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"{cls.__name__:>22} {precision:>5} {dt / n_steps * 1e3:>9.2f} {bench.PER_GPU_BATCH * n_steps / dt:>10.2f}",
                  flush=True)
            del t, batch
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="also time this many full train steps per trainer and precision")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    if not args.no_kernels:
        kernels()
    if args.steps > 0:
        steps(args.steps, args.warmup)


if __name__ == "__main__":
    main()
