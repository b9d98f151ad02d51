"""Per-level time of TopKLoss and DC_and_topk (csrc/loss_topk.hip) against mvd_dcce_fwd / mvd_dcce_finalize /
mvd_dcce_bwd at the same shapes in the same process: the C entry points called back to back on the current stream, HIP
events around each group, median (min, max) of 30 after 5 warm-up calls.  Shapes [2,5,128^3] and [2,5,64^3], random logits
and all logits zero (every CE equal: one histogram bin at every pass, the LDS-contention worst case).

usage: python tools/bench_topk.py [OUT.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_mvd_seg_amd import _lib, ops  # noqa: E402
from multimodal_mvd_seg_amd.ops import _Workspace, _p, _stream, call, query  # noqa: E402

DEV = torch.device("cuda:0")
_lib.load()


def timed(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def run(shape, N=2, K=5, zero_logits=False):
    torch.manual_seed(0)
    x = (torch.zeros if zero_logits else torch.randn)((N, K, *shape), device=DEV) * 2
    t = torch.randint(0, K, (N, 1, *shape), device=DEV).float().reshape(N, -1).contiguous()
    V = t.shape[1]
    n = N * V
    k = ops.topk_count(n, 10)
    g = torch.ones((), device=DEV)
    dl = torch.empty_like(x)
    stats = torch.empty((N, 3 * K + 1), device=DEV)
    loss3 = torch.empty((4,), device=DEV)
    coef = torch.empty((N, K, 2), device=DEV)
    ce = torch.empty((N, V), device=DEV)
    state = torch.empty((4,), dtype=torch.int32, device=DEV)
    loss2 = torch.empty((2,), device=DEV)
    ws = _Workspace.get(max(query("mvd_dcce_workspace_bytes", N, V, K), query("mvd_topk_workspace_bytes", N, V)), DEV)
    s = _stream()

    def dcce_fwd(w_ce=1.0):
        call("mvd_dcce_fwd", _p(x), _p(t), _p(stats), N, V, K, _p(ws), ws.numel(), s)
        call("mvd_dcce_finalize", _p(stats), N, _p(stats), N, _p(loss3), _p(coef), V, K, 0, 0, 1e-5, w_ce, 1.0, s)

    def dcce_bwd():
        call("mvd_dcce_bwd", _p(x), _p(t), _p(coef), _p(g), 1.0, _p(dl), N, V, K, 1.0, s)

    def ce_fwd():
        call("mvd_topk_ce_fwd", _p(x), _p(t), _p(ce), N, V, K, -100, 0.0, s)

    def select():
        call("mvd_topk_select", _p(ce), n, k, _p(state), _p(ws), ws.numel(), s)

    def finalize(dice=None):
        call("mvd_topk_finalize", _p(ce), n, k, _p(state), 1.0, _p(dice), _p(loss2), _p(ws), ws.numel(), s)

    def bwd(cf=None):
        call("mvd_topk_bwd", _p(x), _p(t), _p(ce), _p(state), _p(cf), _p(g), 1.0, _p(dl), N, V, K, k, 1.0, -100, 0.0, s)

    def topk_all():
        ce_fwd(), select(), finalize(), bwd()

    def dctopk_all():
        dcce_fwd(0.0), ce_fwd(), select(), finalize(loss3), bwd(coef)

    def dcce_all():
        dcce_fwd(), dcce_bwd()

    out = {}
    for name, fn in (("dcce fwd+finalize+bwd", dcce_all), ("dcce fwd+finalize", dcce_fwd), ("dcce bwd", dcce_bwd),
                     ("topk fwd+bwd", topk_all), ("dc_and_topk fwd+bwd", dctopk_all), ("topk ce_fwd", ce_fwd),
                     ("topk select (reset + 3 x (hist + scan))", select), ("topk finalize (sum + finish)", finalize),
                     ("topk bwd", bwd)):
        out[name] = timed(fn)
    # again in the other order: the spread between the two visits is the noise of this job
    out["dcce fwd+finalize+bwd (2nd visit)"] = timed(dcce_all)
    out["topk fwd+bwd (2nd visit)"] = timed(topk_all)
    return out


res = {}
for shape in ((128, 128, 128), (64, 64, 64)):
    for zero in (False, True):
        key = f"[2,5,{shape[0]}^3]" + (" all logits zero" if zero else "")
        res[key] = run(shape, zero_logits=zero)
        print(key)
        for k_, (med, lo, hi) in res[key].items():
            print(f"  {k_:46s} median {med:8.1f} us  (min {lo:8.1f}, max {hi:8.1f})")
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
