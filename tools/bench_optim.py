"""Time of the fused optimizer entry points on flat fp32 buffers at the bench.py network's parameter count: mvd_adam_step as
AdamW + amsgrad (36 B / parameter) and as Adam (28 B), and in the same session mvd_sgd_nesterov_step_dev (20 B), whose
achieved bandwidth is the yardstick.  Each call is timed WITHOUT mvd_grad_sumsq (4 B / parameter more, the same for all).

HIP events around REPS back-to-back calls after a warm-up, median of 7 rounds, per call; TB/s on the algorithmic bytes.

--steps: additionally time full train steps of nnUNetTrainerAdamMI355 and nnUNetTrainerMI355 at the bench.py workload
(4 x 128^3, batch 2) in fp32 and bf16: --warmup untimed steps, then --steps timed ones."""
import argparse
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_mvd_seg_amd import _lib  # noqa: E402

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


def bench_parameter_count():
    """FlatParams.numel of the bench.py network (per-tensor padding included), counted on the host."""
    import bench
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(bench.PATCH, bench.STRIDES, batch_size=bench.PER_GPU_BATCH)
    pm = trainer.PlansManager(plans)
    net = trainer.get_network_from_plans(pm, bench.dataset_json(), pm.get_configuration("3d_fullres"),
                                         len(bench.dataset_json()["channel_names"]))
    seen, n = set(), 0
    for p in net.parameters():
        if id(p) not in seen:
            seen.add(id(p))
            n += (p.numel() + 3) // 4 * 4
    return n


def kernels(n):
    dev = torch.device("cuda:0")
    p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 0.01
    m, v, vmax, buf = (torch.zeros(n, device=dev) for _ in range(4))
    sumsq = torch.ones(1, device=dev)
    hyper = torch.zeros(16, dtype=torch.float64, device=dev)
    hyper[:8].copy_(torch.tensor([1e-2, 0.9, 0.999, 1e-8, 3e-5, 12.0, 1.0, 0.0], dtype=torch.float64))
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    sgd_hyper = torch.tensor([1e-2, 0.99, 3e-5, 12.0, 1.0, 0.0], device=dev)
    runs = [("adamw+amsgrad", 36, lambda: _lib.call("mvd_adam_step", _p(p), _p(g), _p(m), _p(v), _p(vmax), _p(sumsq), n,
                                                    _p(hyper), _p(step), 1, _st())),
            ("adam", 28, lambda: _lib.call("mvd_adam_step", _p(p), _p(g), _p(m), _p(v), None, _p(sumsq), n, _p(hyper),
                                           _p(step), 0, _st())),
            ("sgd nesterov", 20, lambda: _lib.call("mvd_sgd_nesterov_step_dev", _p(p), _p(g), _p(buf), _p(sumsq), n,
                                                   _p(sgd_hyper), _st()))]
    print(f"n = {n} parameters ({n * 4 / 1e6:.1f} MB per buffer)")
    print(f"{'call':>14} {'B/param':>8} {'ms':>9} {'TB/s':>7}")
    for name, bpp, run in runs:
        ms = _time(run)
        print(f"{name:>14} {bpp:>8} {ms:>9.4f} {bpp * n / (ms * 1e-3) / 1e12:>7.3f}", flush=True)


def steps(n_steps, warmup):
    import bench
    from multimodal_mvd_seg_amd import trainer
    dev = torch.device("cuda:0")
    print(f"{'trainer':>24} {'prec':>5} {'ms/step':>9} {'samples/s':>10}")
    for precision in ("fp32", "bf16"):
        for cls in (trainer.nnUNetTrainerMI355, trainer.nnUNetTrainerAdamMI355):
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
            print(f"{cls.__name__:>24} {precision:>5} {dt / n_steps * 1e3:>9.2f} {bench.PER_GPU_BATCH * n_steps / dt:>10.2f}",
                  flush=True)
            del t, batch
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="also time this many full train steps per trainer and precision")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--n", type=int, nargs="*", default=[], help="further buffer lengths to time the kernels at (the footprint "
                    "of a call, n x B/param, decides how much of it the 256 MB Infinity Cache holds between calls)")
    args = ap.parse_args()
    if not args.no_kernels:
        for n in [bench_parameter_count()] + args.n:
            kernels(n)
            torch.cuda.empty_cache()
    if args.steps > 0:
        steps(args.steps, args.warmup)


if __name__ == "__main__":
    main()
