"""Time of the residual-encoder kernels and of a ResidualEncoderUNet train step.

Kernels, at one large layer [2, 32, 128^3] fp32: the block tail in its two forms (ops.ResidualAddNormActFn's entry points
mvd_resblock_fwd / _bwd) and the skip branch's pool (mvd_avgpool3d_fwd / _bwd), each against the unfused chain of the
project's own kernels plus torch element-wise ops -- InstanceNorm apply with slope 1 (mvd_instnorm_lrelu_fwd) per normalised
tensor, torch add, torch leaky_relu; for the pool torch's avg_pool3d on the same channels-last tensor.  HIP events around REPS
back-to-back calls after a warm-up, median of 7 rounds, per call; TB/s on the bytes the FUSED form has to move (derived from
shapes, stated per row).

--steps K: full fp32 train steps of nnUNetTrainerMI355 on the ResEnc planner's default network (features 32..320, blocks
(1, 3, 4, 6, 6, 6), decoder (1,) * 5, patch 128^3, batch 2, one input channel), eager and graphed: --warmup untimed steps,
then K timed ones between two HIP events."""
import argparse
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_mvd_seg_amd import _lib  # noqa: E402
from multimodal_mvd_seg_amd._lib import i3  # noqa: E402

N, C, S = 2, 32, (128, 128, 128)
REPS = 10
CL = torch.channels_last_3d


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


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
    return sorted(ts)[len(ts) // 2], ts


def kernels():
    if not torch.cuda.is_available():
        raise SystemExit("bench_resenc: needs an MI355X (no CPU path, nothing is timed without one)")
    dev = torch.device("cuda:0")
    V = S[0] * S[1] * S[2]
    elems = N * V * C
    mk = lambda: torch.randn(N, C, *S, device=dev).contiguous(memory_format=CL)
    a, r, dy = mk(), mk(), mk()
    y, da, dr, t1, t2 = (torch.empty_like(a) for _ in range(5))
    ga, ba, gr, br = (torch.rand(C, device=dev) + 0.5 for _ in range(4))
    dga, dba, dgr, dbr = (torch.empty(C, device=dev) for _ in range(4))
    ma, sa, mr, sr = (torch.empty(N, C, device=dev) for _ in range(4))
    nb = max(_lib.query("mvd_resblock_workspace_bytes", N, V, C), _lib.query("mvd_instnorm_workspace_bytes", N, V, C))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def fused_fwd(proj):
        _lib.call("mvd_resblock_fwd", _p(a), _p(ga), _p(ba), _p(r), _p(gr if proj else None), _p(br if proj else None), _p(y),
                  _p(ma), _p(sa), _p(mr if proj else None), _p(sr if proj else None), N, V, C, 1e-5, 0.01, 0, _p(ws), nb, _st())

    def fused_bwd(proj, acc=0):
        _lib.call("mvd_resblock_bwd", _p(a), _p(r), _p(dy), _p(ga), _p(ba), _p(ma), _p(sa), _p(gr if proj else None),
                  _p(br if proj else None), _p(mr if proj else None), _p(sr if proj else None), _p(da), _p(dr), _p(dga), _p(dba),
                  _p(dgr if proj else None), _p(dbr if proj else None), acc, N, V, C, 0.01, _p(ws), nb, _st())

    def norm_only(x, g, b, out, m, s):   # InstanceNorm apply with slope 1: the project's kernel without an activation
        _lib.call("mvd_instnorm_lrelu_fwd", _p(x), _p(g), _p(b), _p(out), _p(m), _p(s), N, V, C, 1e-5, 1.0, _p(ws), nb, _st())

    def chain_fwd(proj):
        norm_only(a, ga, ba, t1, ma, sa)
        if proj:
            norm_only(r, gr, br, t2, mr, sr)
        torch.add(t1, t2 if proj else r, out=t1)
        F.leaky_relu(t1, 0.01, inplace=True)

    rows = []
    # bytes of the fused forms: forward = statistics reads (1 or 2 tensors) + a, r in + y out; backward = two passes over
    # a, r, dy + da, dr out (+ dr in when accumulating)
    for proj in (False, True):
        name = "projection" if proj else "identity"
        rows.append((f"tail fwd {name} fused", _time(lambda: fused_fwd(proj)), (4 + proj) * 4 * elems))
        rows.append((f"tail fwd {name} chain", _time(lambda: chain_fwd(proj)), (4 + proj) * 4 * elems))
        fused_fwd(proj)
        rows.append((f"tail bwd {name} fused", _time(lambda: fused_bwd(proj)), 8 * 4 * elems))
    fused_fwd(False)
    rows.append(("tail bwd identity fused, accumulate", _time(lambda: fused_bwd(False, 1)), 9 * 4 * elems))
    # pool, stride 2: x in + y out = 1.125 passes
    st = (2, 2, 2)
    yp = torch.empty(N, C, *[e // 2 for e in S], device=dev).contiguous(memory_format=CL)
    dyp = torch.randn_like(yp)
    pool_bytes = int(1.125 * 4 * elems)
    rows.append(("avgpool fwd", _time(lambda: _lib.call("mvd_avgpool3d_fwd", _p(a), _p(yp), N, *S, C, i3(st), _st())), pool_bytes))
    rows.append(("avgpool fwd torch", _time(lambda: F.avg_pool3d(a, st, st)), pool_bytes))
    rows.append(("avgpool bwd", _time(lambda: _lib.call("mvd_avgpool3d_bwd", _p(dyp), _p(da), N, *S, C, i3(st), 0, _st())),
                 pool_bytes))
    rows.append(("avgpool bwd accumulate", _time(lambda: _lib.call("mvd_avgpool3d_bwd", _p(dyp), _p(da), N, *S, C, i3(st), 1,
                                                                   _st())), int(2.125 * 4 * elems)))
    print(f"layer [{N}, {C}, {S[0]}^3] fp32, {elems * 4 / 2 ** 20:.0f} MiB per tensor; median of 7 rounds of {REPS} calls")
    print(f"{'call':>38} {'ms':>9} {'min..max':>17} {'GB (fused form)':>16} {'TB/s':>7}")
    for name, (ms, ts), nbytes in rows:
        print(f"{name:>38} {ms:>9.4f} {min(ts):>8.4f}..{max(ts):<8.4f} {nbytes / 1e9:>16.3f} {nbytes / (ms * 1e-3) / 1e12:>7.3f}",
              flush=True)


def steps(n_steps, warmup):
    from multimodal_mvd_seg_amd import trainer
    dev = torch.device("cuda:0")
    strides = [[1, 1, 1]] + [[2, 2, 2]] * 5
    dataset_json = {"channel_names": {"0": "m0"}, "labels": {"background": 0, "a": 1, "b": 2}}
    print(f"ResidualEncoderUNet, features 32..320, blocks (1, 3, 4, 6, 6, 6), decoder (1,) * 5, patch 128^3, batch 2, fp32; "
          f"{warmup} warm-up steps, {n_steps} timed")
    print(f"{'mode':>8} {'ms/step':>9} {'samples/s':>10}")
    for graph in (False, True):
        plans = trainer.make_plans((128, 128, 128), strides, batch_size=2, unet_class_name='ResidualEncoderUNet',
                                   n_blocks_per_stage=(1, 3, 4, 6, 6, 6), n_conv_per_stage_decoder=(1,) * 5)
        t = trainer.nnUNetTrainerMI355(plans, "3d_fullres", 0, dataset_json, device=dev)
        t.use_hip_graph = graph
        torch.manual_seed(0)
        t.initialize()
        batch = t.make_dummy_batch()
        t.on_train_epoch_start()
        t.hip_graph_warmup = min(t.hip_graph_warmup, max(1, warmup - 2))
        for _ in range(warmup):
            t.train_step(batch)
        torch.cuda.synchronize()
        if graph:
            assert t._step_graph is not None and t._step_graph["graph"] is not None, "the step was never captured"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_steps):
            t.train_step(batch)      # (each step ends with the loss read back, as the reference's does)
        e1.record()
        torch.cuda.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        print(f"{'graphed' if graph else 'eager':>8} {dt / n_steps * 1e3:>9.2f} {2 * n_steps / dt:>10.2f}", flush=True)
        del t, batch
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="also time this many full train steps, eager and graphed")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    if not args.no_kernels:
        kernels()
    if args.steps > 0:
        steps(args.steps, args.warmup)


if __name__ == "__main__":
    main()
