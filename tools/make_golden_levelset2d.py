"""Generates tests/golden/levelset2d_diagrams.npz and tests/golden/topoloss_*.npz (build container only, like
tools/make_golden.py: it needs the reference tree and its C++ persistence extension compiled into oracle/_ref).

What computes the expected values is the reference's own code: the compiled extension (persistenceForwardHom,
persistenceBackward) and the bodies of init_freudenthal_2d, LevelSetLayer / LevelSetLayer2D, SubLevelSetDiagram,
TopKBarcodeLengths and TopoLoss, executed out of the reference's files (make_golden.ref_function).  `topologylayer` is
not importable as a package: the names those bodies import from it are bound here to the compiled module.

usage: python tools/make_golden_levelset2d.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import ref_function, save  # noqa: E402
from oracle import build_ref  # noqa: E402

TL = "training/topologylayer/"


def reference_stack():
    m = build_ref.load()
    assert m is not None, "run `python oracle/build_ref.py` first"
    ns = {"nn": nn, "SimplicialComplex": m.SimplicialComplex, "persistenceForwardHom": m.persistenceForwardHom,
          "persistenceForwardCohom": m.persistenceForwardCohom, "persistenceBackward": m.persistenceBackward,
          "Function": torch.autograd.Function}
    src = {}
    for rel, names in ((TL + "functional/sublevel.py", ["SubLevelSetDiagram"]),
                       (TL + "nn/levelset.py", ["init_freudenthal_2d", "LevelSetLayer", "LevelSetLayer2D"]),
                       (TL + "nn/features.py", ["get_start_end", "get_raw_barcode_lengths", "get_barcode_lengths", "pad_k",
                                                "TopKBarcodeLengths"]),
                       ("training/loss/Topo_Loss.py", ["TopoLoss"])):
        for name in names:
            obj, where = ref_function(rel, name, **ns)
            # the bodies look their helpers up in their own globals: share one namespace
            ns[name] = obj
            obj_globals = getattr(obj, "__globals__", None)
            if obj_globals is not None:
                obj_globals.update(ns)
            src[name] = where
    # classes hold their methods' globals: refresh all of them with the final namespace
    for name in src:
        obj = ns[name]
        fns = [obj] if hasattr(obj, "__globals__") else [v for v in vars(obj).values()]
        for f in fns:
            f = getattr(f, "__func__", f)
            if hasattr(f, "__globals__"):
                f.__globals__.update(ns)
    return m, ns, src


def srt(a):
    return a[np.lexsort(tuple(a[:, c] for c in range(a.shape[1] - 1, -1, -1)))]


def critical_vertices(m, X, dgms):
    """(birth vertex, death vertex) of every bar, read through persistenceBackward with one-hot gradients."""
    out = []
    for k, dgm in enumerate(dgms):
        crit = np.full((dgm.shape[0], 2), -1, dtype=np.int64)
        for j in range(dgm.shape[0]):
            for col in range(2):
                if not np.isfinite(float(dgm[j, col])):
                    continue
                gs = [torch.zeros_like(d) for d in dgms]
                gs[k][j, col] = 1.0
                crit[j, col] = int(torch.argmax(m.persistenceBackward(X, gs)))
        out.append(crit)
    return out


def diagram_fixtures(m, ns):
    rng = np.random.default_rng(32)
    arrs = {"source": "reference C++ persistence (hom.cpp, cohom.cpp:148-196) compiled into oracle/_ref, on "
                      "init_freudenthal_2d and LevelSetLayer2D executed out of nn/levelset.py; for W == 1 or H == 1 the "
                      "reference is run with maxdim 0 (its maxdim-1 bookkeeping indexes a dimension the complex does not "
                      "have) and dgm1 is the empty diagram numPairs(1) = E - V + 1 = 0 prescribes; the single vertex of 1x1 is "
                      "written by hand (one essential bar, hom.cpp:155-185): without edges the reference indexes an empty "
                      "backprop_lookup"}
    names = []
    for (W, H), quarters in (((1, 1), False), ((1, 5), False), ((5, 1), False), ((2, 2), False), ((3, 2), False),
                             ((5, 4), False), ((8, 8), True), ((7, 9), True), ((16, 12), False), ((32, 32), False)):
        f = rng.standard_normal((H, W)).astype(np.float32)
        if quarters:
            f = (np.round(f * 4) / 4).astype(np.float32)
        else:
            assert np.unique(f).size == f.size
        name = f"{W}x{H}"
        names.append(name)
        arrs[name + "/f"] = f
        arrs[name + "/tie_free"] = np.array(not quarters)
        maxdim = 1 if (W > 1 and H > 1) else 0
        for sub in (True, False):
            if W * H == 1:
                # a complex without edges makes the reference index backprop_lookup[0] of an empty vector: the one bar of
                # a single vertex is written down by hand (hom.cpp:155-185: an unpaired vertex is an essential bar)
                tag = name + ("/sub" if sub else "/super")
                arrs[f"{tag}/dgm0"] = np.array([[f[0, 0], np.inf if sub else -np.inf, 0, -1]], dtype=np.float32)
                arrs[f"{tag}/dgm1"] = np.zeros((0, 4), dtype=np.float32)
                continue
            layer = ns["LevelSetLayer2D"](size=(W, H), maxdim=maxdim, sublevel=sub)
            dgms, issub = layer(torch.from_numpy(f.copy()))
            assert issub == sub
            dgms = [d.detach().clone() for d in dgms]
            tag = name + ("/sub" if sub else "/super")
            crit = critical_vertices(m, layer.complex, dgms) if not quarters else [None] * len(dgms)
            for k in range(2):
                if k < len(dgms):
                    d = dgms[k].numpy().astype(np.float32)
                    rows = np.concatenate([d, crit[k].astype(np.float32)], 1) if crit[k] is not None else d
                else:
                    rows = np.zeros((0, 4 if not quarters else 2), dtype=np.float32)
                arrs[f"{tag}/dgm{k}"] = srt(rows) if rows.shape[0] else rows
            T = 2 * (W - 1) * (H - 1)
            assert arrs[f"{tag}/dgm0"].shape[0] == W * H and arrs[f"{tag}/dgm1"].shape[0] == T
    arrs["names"] = np.array(names)
    save("levelset2d_diagrams.npz", **arrs)


def topoloss_fixtures(m, ns):
    TopK, TopoLoss = ns["TopKBarcodeLengths"], ns["TopoLoss"]
    B, C, idx = 2, 3, [0, 1]
    for (W, H), seed in (((5, 4), 1), ((16, 12), 2), ((32, 32), 3)):
        for attempt in range(50):   # the first seed of the sequence whose fields and bar lengths are tie-free
            try:
                _topoloss_fixture(m, ns, TopK, TopoLoss, B, C, idx, W, H, seed + 10 * attempt)
                break
            except AssertionError as e:
                print(f"  {W}x{H} seed {seed + 10 * attempt}: {e}")
        else:
            raise RuntimeError("no tie-free field found")


def _topoloss_fixture(m, ns, TopK, TopoLoss, B, C, idx, W, H, seed):
    g = torch.Generator().manual_seed(seed)
    y_pred = torch.softmax(2.0 * torch.randn((B, C, H, W), generator=g), 1).contiguous()
    y_raw = torch.softmax(2.0 * torch.randn((B, C, H, W), generator=g), 1).contiguous()
    arrs = {"source": "TopoLoss / TopKBarcodeLengths / LevelSetLayer2D executed out of the reference's files on its "
                      "compiled C++ persistence extension", "y_pred": y_pred, "y_raw": y_raw, "idx": np.array(idx), "seed": np.array(seed)}
    for max_k in (5, 20):
        loss = TopoLoss(img_size=(W, H), topo_weight=1, sqdiff_weight=10, max_k=max_k)
        # top-k lengths and the number of non-zero bars of every problem
        topk = np.zeros((B, len(idx), 2, max_k), dtype=np.float32)
        nz = np.zeros((B, len(idx), 2), dtype=np.int64)
        for b in range(B):
            for n, i in enumerate(idx):
                plane = y_pred[b, i + 1]
                assert torch.unique(plane).numel() == plane.numel(), "field is not tie-free"
                info = loss.dgminfo(plane)
                for dim in range(2):
                    lens = ns["get_barcode_lengths"](info[0][dim].detach().clone(), info[1])
                    top = torch.sort(lens, descending=True)[0][:max_k + 1]
                    pos = top[top > 0]
                    assert torch.unique(pos).numel() == pos.numel(), "top k+1 lengths are not distinct"
                    topk[b, n, dim] = TopK(dim=dim, k=max_k)(info).detach().numpy()
                    nz[b, n, dim] = int((lens > 0).sum())
        # labels below, at and above the number of non-zero bars (capped by what max_k shows) and above max_k
        label = torch.zeros((B, C, 2), dtype=torch.int64)
        for b in range(B):
            for n, i in enumerate(idx):
                for dim in range(2):
                    shown = min(int(nz[b, n, dim]), max_k)
                    label[b, i, dim] = [max(shown - 1, 0), shown, shown + 1, max_k + 3][(2 * b + n + dim) % 4]
        tag = f"k{max_k}/"
        arrs[tag + "topk"] = topk
        arrs[tag + "nonzero_bars"] = nz
        arrs[tag + "topo_label"] = label
        for with_raw in (True, False):
            loss.sqdiff_weight = 10 if with_raw else 0
            yp = y_pred.clone().requires_grad_(True)
            val = loss(yp, y_raw, label, idx=idx)
            val.backward()
            shared = yp.grad.detach().clone()
            # TopoLoss keeps ONE SimplicialComplex for all its problems, and every forward overwrites the tables
            # persistenceBackward reads (backprop_lookup, function_map): in a batched call the gradients of all problems
            # land on the critical vertices of the LAST one.  Its own comment says the layer works on one sample at a
            # time; the expected gradient is therefore taken that way -- the same bodies, one problem per forward +
            # backward, with the factors of TopoLoss.forward -- and the batched call is kept for the loss value.
            yp = y_pred.clone().requires_grad_(True)
            for b in range(B):
                for i in idx:
                    t = loss._get_l_topo(yp[b:b + 1].clone(), label[b:b + 1].clone(), i)      # batch of one: no mean
                    (loss.topo_weight * (t / B) / len(idx)).backward()
            if with_raw:
                (loss.sqdiff_weight * loss.l2_loss(y_raw, yp)).backward()
            last = (B - 1, idx[-1] + 1)
            assert torch.equal((yp.grad - (shared if not with_raw else yp.grad))[last], torch.zeros(H, W)), \
                "the last problem's gradient is the one the batched call gets right"
            sub = tag + ("with_raw/" if with_raw else "topo_only/")
            arrs[sub + "loss"] = val.detach()
            arrs[sub + "grad"] = yp.grad.detach()
            if not with_raw:
                arrs[sub + "grad_batched_call"] = shared
        # per vertex: sum of |contributions| and number of bars meeting there (persistenceBackward of |d loss / d dgm|)
        scale = 1.0 / len(idx) / B
        gabs = torch.zeros((B, C, H, W))
        gcnt = torch.zeros((B, C, H, W))
        sumsq = 0.0
        for b in range(B):
            for n, i in enumerate(idx):
                plane = y_pred[b, i + 1].clone().requires_grad_(True)
                dgms, issub = loss.dgminfo(plane)
                for d in dgms:
                    d.retain_grad()
                tot = 0
                for dim in range(2):
                    sq = TopK(dim=dim, k=max_k)((dgms, issub)) ** 2
                    sumsq += float(sq.detach().sum())
                    signs = torch.ones(max_k)
                    signs[:label[b, i, dim]] = -1
                    tot = tot + (sq * signs).sum()
                tot.backward()
                ga = [d.grad.abs() for d in dgms]
                X = loss.dgminfo.complex
                gabs[b, i + 1] = m.persistenceBackward(X, ga).view(H, W) * scale
                gcnt[b, i + 1] = m.persistenceBackward(X, [(a != 0).float() for a in ga]).view(H, W)
        arrs[tag + "grad_abs_sum"] = gabs
        arrs[tag + "grad_bars_meeting"] = gcnt
        arrs[tag + "sum_len_sq"] = np.array(sumsq * scale)
    save(f"topoloss_{W}x{H}.npz", **arrs)


if __name__ == "__main__":
    m, ns, src = reference_stack()
    for k, v in src.items():
        print(f"  {k}: {v}")
    diagram_fixtures(m, ns)
    topoloss_fixtures(m, ns)
