"""Timing of the FinalNetv2 bottleneck fusion block (csrc/attention.hip) and of the train step that contains it.

  python tools/bench_fusion.py                 the block alone at B = 2, N = 128, C = 256 and at N = 64, C = 320: HIP-event
                                               time of forward and forward + backward, eager and as one graph replay, and
                                               the launch counts
  python tools/bench_fusion.py --trainers      the dual-branch train step at the cfg-3 plan (patch 128^3, six stages, batch
                                               2, 2 modalities): FinalNetTrainerMI355 and ContrastiveTrainerMI355 in one
                                               process, alternating; the block's share of the FinalNetv2 step

Prints one JSON line per measurement.  Times are medians over `--reps` repetitions, in microseconds (block) or
milliseconds (step).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from multimodal_mvd_seg_amd import network, ops, trainer  # noqa: E402

DEV = torch.device("cuda:0")
LAUNCHES = {"mvd_attention_bwd": 2, "mvd_linear_bwd": 2}   # kernels per entry point where it is not one


def count_launches(fn):
    counts, real = {"n": 0}, ops.call

    def counting(name, *a):
        counts["n"] += LAUNCHES.get(name, 1)
        return real(name, *a)
    ops.call = counting
    try:
        fn()
    finally:
        ops.call = real
    return counts["n"]


def event_time_us(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def bench_block(B, sp, C, reps):
    N = sp[0] * sp[1] * sp[2]
    torch.manual_seed(0)
    fus = network.BottleneckFusion(C, N).to(DEV).train()
    mk = lambda: torch.randn(B, *sp, C, device=DEV).permute(0, 4, 1, 2, 3).requires_grad_(True)
    x1, x2 = mk(), mk()
    g1, g2 = torch.randn_like(x1), torch.randn_like(x2)

    def fwd():
        with torch.no_grad():
            return fus(x1, x2)

    def fwd_bwd():
        for p in [x1, x2] + list(fus.parameters()):
            p.grad = None   # (fresh gradients: no accumulation kernels of autograd in the timing)
        y1, y2 = fus(x1, x2)
        torch.autograd.backward([y1, y2], [g1, g2])
    out = {"shape": {"B": B, "N": N, "C": C}, "launches_forward": count_launches(fwd)}
    out["launches_forward_backward"] = count_launches(fwd_bwd)
    for name, fn in (("forward", fwd), ("forward_backward", fwd_bwd)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out[name + "_eager_us"] = round(event_time_us(fn, reps), 1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        out[name + "_graph_us"] = round(event_time_us(g.replay, reps), 1)
    print(json.dumps({"fusion_block": out}), flush=True)
    return out


def bench_trainers(rounds, steps):
    dj = {"channel_names": {"0": "mod0", "1": "mod1"}, "labels": {"background": 0, **{f"c{i}": i for i in range(1, 5)}}}
    plans = trainer.make_plans((128, 128, 128), [[1, 1, 1]] + [[2, 2, 2]] * 5, batch_size=2)
    trs = {}
    for name in ("FinalNetTrainerMI355", "ContrastiveTrainerMI355"):
        t = getattr(trainer, name)(plans, "3d_fullres", 0, dj, device=DEV)
        t.use_topo = False   # cfg 3: the mutual-distillation step without the topology term
        torch.manual_seed(0)
        t.initialize()
        t.on_train_epoch_start()
        batch = t.make_dummy_batch()
        for _ in range(t.hip_graph_warmup + 3):
            t.train_step(batch)
        torch.cuda.synchronize()
        trs[name] = (t, batch)
    times = {n: [] for n in trs}
    for _ in range(rounds):
        for n, (t, batch) in trs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                t.train_step(batch, return_device_loss=True)
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) / steps)
    res = {n: {"step_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
           for n, v in times.items()}
    print(json.dumps({"train_step_cfg3_plan": res, "rounds": rounds, "steps_per_round": steps}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trainers", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fusion.py needs an MI355X"
    bench_block(2, (2, 8, 8), 256, args.reps)
    small = bench_block(2, (4, 4, 4), 320, args.reps)
    if args.trainers:
        res = bench_trainers(args.rounds, args.steps)
        step = res["FinalNetTrainerMI355"]["step_ms"]
        print(json.dumps({"fusion_block_share_of_step": round(small["forward_backward_graph_us"] / 1e3 / step, 4)}),
              flush=True)


if __name__ == "__main__":
    main()
