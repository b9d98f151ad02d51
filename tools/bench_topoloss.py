"""Times the persistence topological loss (losses.TopoLoss) at B = 2, 3 foreground classes, max_k = 20 on 128x128 and
256x256 probability maps: forward and backward, the forward split into keys + sort (device events), the D2H copy, the host
pairing sweep, the H2D copy (host timers around synchronised copies) and the rest (top-k, loss kernels).

    python tools/bench_topoloss.py                 # on the MI355X
    python tools/bench_topoloss.py --reference     # the reference's per-problem cost, where oracle/_ref is built (no GPU)

--reference times, per problem, SimplicialComplex.extendFloat + persistenceForwardHom(maxdim 1) of the reference's compiled
C++ on the same fields, summed over the same P = 6 problems; the complex is built once outside the timing, as the
reference's layer does.  The two sides run on different hosts: no ratio is asserted anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, IDX, MAX_K = 2, 4, [0, 1, 2], 20
SIZES = (128, 256)


def fields(size):
    g = torch.Generator().manual_seed(size)
    # a smooth map plus noise: probabilities of a network, not white noise
    low = torch.randn((B, C, size // 8, size // 8), generator=g)
    x = torch.nn.functional.interpolate(low, size=(size, size), mode="bilinear") * 3 + 0.3 * torch.randn((B, C, size, size), generator=g)
    return torch.softmax(x, 1).contiguous()


def bench_device(steps, warmup):
    from multimodal_mvd_seg_amd import losses, ops
    dev = torch.device("cuda:0")
    for size in SIZES:
        y = fields(size).to(dev)
        label = losses.betti_topo_label((y.argmax(1, keepdim=True)).float(), C)[:, 1:].contiguous()
        loss = losses.TopoLoss((size, size), sqdiff_weight=0, max_k=MAX_K)
        rows = []
        for it in range(warmup + steps):
            yp = y.clone().requires_grad_(True)
            ops.Ls2dTimes.on = True
            torch.cuda.synchronize()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            t0 = time.perf_counter()
            l = loss(yp, None, label, idx=IDX)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            e[0].record()
            l.backward()
            e[1].record()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ops.Ls2dTimes.on = False
            r = dict(ops.Ls2dTimes.last)
            r["forward_ms"] = (t1 - t0) * 1e3
            r["forward_rest_ms"] = r["forward_ms"] - sum(r[k] for k in ("keys_sort_ms", "d2h_ms", "host_sweep_ms", "h2d_ms"))
            r["backward_device_ms"] = e[0].elapsed_time(e[1])
            r["backward_ms"] = (t2 - t1) * 1e3
            if it >= warmup:
                rows.append(r)
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        med["host_sweep_share_of_forward"] = med["host_sweep_ms"] / med["forward_ms"]
        print(json.dumps({"size": size, "problems": B * len(IDX), "max_k": MAX_K, "steps": steps,
                          **{k: round(v, 4) for k, v in med.items()}}))


def bench_reference(repeats):
    from oracle import build_ref
    m = build_ref.load()
    assert m is not None, "oracle/_ref is not built"
    for size in SIZES:
        W = H = size
        s = m.SimplicialComplex()
        for i in range(H * W):
            s.append([i])
        for i in range(H):
            for j in range(W - 1):
                s.append([i * W + j, i * W + j + 1])
        for i in range(H - 1):
            for j in range(W):
                s.append([i * W + j, (i + 1) * W + j])
        for i in range(H - 1):
            for j in range(W - 1):
                a = i * W + j
                s.append([a, a + W + 1])
                s.append([a, a + 1, a + W + 1])
                s.append([a, a + W, a + W + 1])
        s.initialize()
        y = fields(size)
        tot = []
        for _ in range(repeats):
            t = 0.0
            for b in range(B):
                for i in IDX:
                    f = (-y[b, i + 1]).reshape(-1).contiguous()
                    t0 = time.perf_counter()
                    s.extendFloat(f)
                    m.persistenceForwardHom(s, 1, 0)
                    t += time.perf_counter() - t0
            tot.append(t * 1e3)
        print(json.dumps({"size": size, "problems": B * len(IDX), "reference_extend_plus_hom_ms": round(float(np.median(tot)), 2),
                          "repeats": repeats}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    if a.reference:
        bench_reference(a.repeats)
    else:
        bench_device(a.steps, a.warmup)
