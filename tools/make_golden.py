"""Generates tests/golden/* (run in the BUILD container only: it imports reference modules by file path from
/root/reference and the reference's C++ persistence extension compiled into oracle/_ref).

Each fixture holds inputs + expected outputs (data only).  `source` in every file says what produced the
expected values: "reference" = a module of /root/reference executed here; "oracle" = this repo's CPU
restatement (the reference's own module is not importable -- SURVEY.md 8c).

usage: python tools/make_golden.py
"""
import ast
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import unet_oracle as UO, loss_oracle as LO, step_oracle as SO, cc_oracle, build_ref  # noqa: E402

R = "/root/reference/nnUNet/nnunetv2"
OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)


def ref_module(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(R, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def save(name, **arrs):
    np.savez_compressed(os.path.join(OUT, name), **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v))
                                                     for k, v in arrs.items()})
    print("wrote", name)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ conv3d (torch CPU ops = reference arithmetic)
def conv_fixtures():
    for tag, stride in (("s1", (1, 1, 1)), ("s2", (2, 2, 2)), ("s122", (1, 2, 2))):
        for cin, cout in ((1, 32), (4, 32), (32, 64)):
            g = gen(10 + cin)
            x = torch.randn(2, cin, 12, 10, 14, generator=g, dtype=torch.float64, requires_grad=True)
            w = (torch.randn(cout, cin, 3, 3, 3, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
            b = (torch.randn(cout, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
            y = F.conv3d(x, w, b, stride, 1)
            gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
            y.backward(gy)
            save(f"conv3d_{tag}_c{cin}_{cout}.npz", source="torch.nn.functional.conv3d fp64 (CPU)",
                 stride=stride, x=x.float(), w=w.float(), b=b.float(), y=y.float(), gy=gy.float(),
                 gx=x.grad.float(), gw=w.grad.float(), gb=b.grad.float())
    for tag, st, cin, cout, sp in (("k2s2", (2, 2, 2), 96, 40, (3, 4, 5)), ("k122s122", (1, 2, 2), 64, 32, (3, 4, 5)),
                                   ("k2s2_small", (2, 2, 2), 8, 4, (4, 3, 5))):
        g = gen(20)
        x = torch.randn(2, cin, *sp, generator=g, dtype=torch.float64, requires_grad=True)
        w = (torch.randn(cin, cout, *st, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
        b = (torch.randn(cout, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
        y = F.conv_transpose3d(x, w, b, st)
        gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(gy)
        save(f"convT3d_{tag}.npz", source="torch.nn.functional.conv_transpose3d fp64 (CPU)", stride=st,
             x=x.float(), w=w.float(), b=b.float(), y=y.float(), gy=gy.float(), gx=x.grad.float(),
             gw=w.grad.float(), gb=b.grad.float())
    # 1x1x1 seg head
    g = gen(21)
    x = torch.randn(2, 32, 5, 6, 7, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(5, 32, 1, 1, 1, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
    b = (torch.randn(5, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
    y = F.conv3d(x, w, b)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    save("conv1x1.npz", source="torch conv3d k=1 fp64 (CPU)", x=x.float(), w=w.float(), b=b.float(), y=y.float(),
         gy=gy.float(), gx=x.grad.float(), gw=w.grad.float(), gb=b.grad.float())


def instnorm_fixtures():
    g = gen(30)
    x = (torch.randn(2, 5, 7, 9, 11, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_()
    gamma = (torch.rand(5, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    beta = (torch.randn(5, generator=g, dtype=torch.float64) * 0.2).requires_grad_()
    y = F.leaky_relu(F.instance_norm(x, None, None, gamma, beta, True, 0.1, 1e-5), 0.01)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    save("instnorm_lrelu.npz", source="torch instance_norm(eps=1e-5)+leaky_relu(0.01) fp64 (CPU)", x=x.float(),
         gamma=gamma.float(), beta=beta.float(), y=y.float(), gy=gy.float(), gx=x.grad.float(),
         ggamma=gamma.grad.float(), gbeta=beta.grad.float())


# ------------------------------------------------------------------ reference-pinned small modules
def reference_fixtures():
    rce = ref_module("training/loss/robust_ce_loss.py", "ref_rce")
    g = gen(40)
    logits = torch.randn(2, 5, 4, 4, 4, generator=g, requires_grad=True)
    tgt = torch.round(torch.rand(2, 1, 4, 4, 4, generator=g) * 4)
    l = rce.RobustCrossEntropyLoss()(logits, tgt)
    l.backward()
    assert torch.equal(l.detach(), LO.RobustCrossEntropyLoss()(logits.detach(), tgt))
    save("robust_ce.npz", source="reference robust_ce_loss.py:6-16", logits=logits, target=tgt, loss=l,
         glogits=logits.grad)

    sk = ref_module("training/loss/soft_skeleton.py", "ref_skel")
    for shape, binary, seed in (((1, 1, 16, 16, 16), False, 41), ((2, 3, 12, 10, 14), False, 42),
                                ((1, 1, 16, 16, 16), True, 43), ((2, 1, 9, 11, 8), True, 44)):
        for it in (1, 3, 10):
            g = gen(seed)
            x = torch.rand(shape, generator=g)
            if binary:
                # tie-heavy input (blobby binary mask)
                x = (F.avg_pool3d(x, 3, 1, 1) > 0.5).float()
            x.requires_grad_()
            y = sk.soft_skel(x, it)
            gy = torch.randn(y.shape, generator=g)
            y.backward(gy)
            yo = LO.soft_skel(x.detach(), it)
            assert torch.equal(y.detach(), yo), "oracle soft_skel differs from the reference"
            e = sk.soft_erode(x.detach())
            d = sk.soft_dilate(x.detach())
            save(f"soft_skel_{'bin' if binary else 'u'}_{'x'.join(map(str, shape))}_iter{it}.npz",
                 source="reference soft_skeleton.py:6-37", iter=it, x=x, skel=y, gy=gy, gx=x.grad, erode=e, dilate=d)

    poly = ref_module("training/lr_scheduler/polylr.py", "ref_poly")
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], 1e-2)
    # the reference ctor passes a 4th positional arg (`verbose`) that torch 2.10's LRScheduler no longer takes
    # (ordinary TypeError); its step() body (polylr.py:13-20) is what defines the schedule, so run that on a stub
    import types
    sch = types.SimpleNamespace(optimizer=opt, initial_lr=1e-2, max_steps=200, exponent=0.9, ctr=0)
    lrs = []
    for e in range(200):
        poly.PolyLRScheduler.step(sch, e)
        lrs.append(opt.param_groups[0]['lr'])
    assert np.allclose(lrs, [SO.poly_lr(1e-2, e, 200) for e in range(200)], rtol=0, atol=0)
    json.dump({"source": "reference polylr.py:4-20", "initial_lr": 1e-2, "max_steps": 200, "lrs": lrs},
              open(os.path.join(OUT, "polylr.json"), "w"))

    init = ref_module("utilities/network_initialization.py", "ref_init")
    stats = {}
    torch.manual_seed(0)
    for name, mod in (("conv_32_32", torch.nn.Conv3d(32, 32, 3)), ("conv_4_32", torch.nn.Conv3d(4, 32, 3)),
                      ("convT_64_32", torch.nn.ConvTranspose3d(64, 32, 2, 2)), ("conv1_32_5", torch.nn.Conv3d(32, 5, 1))):
        mod.apply(init.InitWeights_He(1e-2))
        fan_in = mod.weight.size(1) * mod.weight[0, 0].numel()
        stats[name] = {"std": float(mod.weight.std()), "expected_std": float(np.sqrt(2 / (1 + 1e-4) / fan_in)),
                       "bias_abs_max": float(mod.bias.abs().max()), "shape": list(mod.weight.shape)}
    json.dump({"source": "reference network_initialization.py:4-12", "stats": stats},
              open(os.path.join(OUT, "he_init_stats.json"), "w"), indent=1)

    topo = ref_module("experiment_planning/experiment_planners/network_topology.py", "ref_topo")
    props = {}
    for name, patch, spacing in (("cfg1", (64, 64, 64), (1, 1, 1)), ("cfg2", (128, 128, 128), (1, 1, 1)),
                                 ("cfg5", (160, 160, 128), (1, 1, 1)), ("author", (64, 128, 256), (1, 1, 1))):
        r = topo.get_pool_and_conv_props(spacing, patch, 4, 999999)
        props[name] = {"patch": list(patch), "num_pool_per_axis": [int(i) for i in r[0]],
                       "pool_op_kernel_sizes": [[int(j) for j in i] for i in r[1]],
                       "conv_kernel_sizes": [[int(j) for j in i] for i in r[2]],
                       "patch_size": [int(i) for i in r[3]], "must_be_divisible_by": [int(i) for i in r[4]]}
    json.dump({"source": "reference network_topology.py:30-105", "props": props},
              open(os.path.join(OUT, "topology_props.json"), "w"), indent=1)
    print("wrote polylr.json he_init_stats.json topology_props.json")


# ------------------------------------------------------------------ reference functions whose MODULE cannot be imported
def ref_function(rel, func_name, class_name=None, **ns):
    """Compiles ONE function definition out of a reference source file and returns it as a live function.  Used for
    pure torch/numpy functions whose module fails at import time on an absent third-party package (other_loss.py ->
    lightly, base_data_loader.py / nnUNetTrainer.py -> batchgenerators, sliding_window_prediction.py -> acvl_utils):
    the function body itself is executed unchanged, so the fixtures below are reference-pinned.  Runs in the build
    container only (needs /root/reference); nothing of the source text is stored."""
    import typing
    path = os.path.join(R, rel)
    tree = ast.parse(open(path).read(), path)
    body = tree.body
    if class_name is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == class_name).body
    # (a ClassDef of that name is picked whole: LabelManager, ConvertSegmentationToRegionsTransform)
    node = next(n for n in body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == func_name)
    node.decorator_list = []
    code = compile(ast.Module(body=[node], type_ignores=[]), path, "exec")
    glob = {"np": np, "torch": torch, "F": F, "Union": typing.Union, "Tuple": typing.Tuple, "List": typing.List}
    glob.update(ns)
    exec(code, glob)
    return glob[func_name], f"{rel}:{node.lineno}-{node.end_lineno}"


def extracted_reference_fixtures():
    import types
    # ---- distill_kl / l2_loss (other_loss.py:51-78); distill_kl carries a stray `self` first parameter
    kl, kl_src = ref_function("training/loss/other_loss.py", "distill_kl")
    l2, l2_src = ref_function("training/loss/other_loss.py", "l2_loss")
    for name, shape, T in (("distill_kl_c5_T1", (2, 5, 6, 6, 6), 1), ("distill_kl_c5_T4", (2, 5, 6, 6, 6), 4),
                           ("distill_kl_c1_T1", (2, 1, 6, 6, 6), 1), ("distill_kl_c1_T4", (2, 1, 6, 6, 6), 4)):
        g = gen(50)
        ys = (torch.randn(shape, generator=g) * 2).requires_grad_()
        yt = (torch.randn(shape, generator=g) * 2).requires_grad_()
        l = kl(None, ys, yt, T)
        l.backward()
        assert torch.equal(l.detach(), LO.distill_kl(ys.detach(), yt.detach(), T)), "oracle distill_kl != reference"
        save(name + ".npz", source="reference " + kl_src, T=T, ys=ys, yt=yt, loss=l, gys=ys.grad, gyt=yt.grad)
    for name, T in (("feat_kl_T1", 1), ("feat_kl_T4", 4)):
        g = gen(51)
        a = torch.randn(2, 32, 5, 6, 4, generator=g, requires_grad=True)
        b = torch.randn(2, 32, 5, 6, 4, generator=g, requires_grad=True)
        l = l2(a, b, True, T)
        l.backward()
        assert torch.equal(l.detach(), LO.l2_loss(a.detach(), b.detach(), True, T)), "oracle l2_loss != reference"
        save(name + ".npz", source="reference " + l2_src, T=T, a=a, b=b, loss=l, ga=a.grad, gb=b.grad)
    g = gen(52)
    a = torch.randn(2, 8, 5, 6, 4, generator=g, requires_grad=True)
    b = torch.randn(2, 8, 5, 6, 4, generator=g, requires_grad=True)
    l = l2(a, b, False)
    l.backward()
    assert torch.equal(l.detach(), LO.l2_loss(a.detach(), b.detach(), False))
    save("l2_loss_plain.npz", source="reference " + l2_src, a=a, b=b, loss=l, ga=a.grad, gb=b.grad)

    # ---- per-rank batch split (nnUNetTrainer.py:304-349): the method on a stub trainer, torch.distributed stubbed
    cases = {}
    for gb in range(2, 17):
        for ws in range(1, 9):
            if gb < ws:
                continue
            bs, ov = [], []
            for rank in range(ws):
                dist_stub = types.SimpleNamespace(get_world_size=lambda ws=ws: ws, get_rank=lambda rank=rank: rank)
                fn, split_src = ref_function("training/nnUNetTrainer/nnUNetTrainer.py", "_set_batch_size_and_oversample",
                                             "nnUNetTrainer", dist=dist_stub, print=lambda *a, **k: None)
                me = types.SimpleNamespace(is_ddp=True, oversample_foreground_percent=0.33,
                                           configuration_manager=types.SimpleNamespace(batch_size=gb))
                fn(me)
                bs.append(int(me.batch_size))
                ov.append(float(me.oversample_foreground_percent))
            o_bs, o_ov = SO.ddp_batch_split(gb, ws)
            assert o_bs == bs and o_ov == ov, (gb, ws, bs, o_bs, ov, o_ov)
            cases[f"{gb}_{ws}"] = {"batch_sizes": bs, "oversample": ov}
    json.dump({"source": "reference " + split_src + " (method executed on a stub trainer per rank)", "cases": cases},
              open(os.path.join(OUT, "ddp_split.json"), "w"))

    # ---- sliding-window step placement and Gaussian importance map (sliding_window_prediction.py:10-56)
    steps, steps_src = ref_function("inference/sliding_window_prediction.py", "compute_steps_for_sliding_window")
    from scipy.ndimage import gaussian_filter
    gauss, gauss_src = ref_function("inference/sliding_window_prediction.py", "compute_gaussian",
                                    gaussian_filter=gaussian_filter)
    sw = []
    for image, tile, step in (((110,), (64,), 0.5), ((128, 128, 128), (128, 128, 128), 0.5),
                              ((192, 256, 256), (128, 128, 128), 0.5), ((133, 160, 201), (64, 96, 128), 0.5),
                              ((70, 70, 70), (64, 64, 64), 1.0), ((100, 300, 77), (48, 160, 64), 0.25),
                              ((65, 64, 200), (64, 64, 64), 0.75)):
        sw.append({"image_size": list(image), "tile_size": list(tile), "tile_step_size": step,
                   "steps": [[int(v) for v in ax] for ax in steps(image, tile, step)]})
    gm = []
    for tile in ((8, 8, 8), (6, 10, 12), (16, 16, 16)):
        m = gauss(tile, 1. / 8, 1000, torch.float32, torch.device("cpu"))
        gm.append({"tile_size": list(tile), "sigma_scale": 0.125, "value_scaling_factor": 1000,
                   "map": [float(v) for v in m.reshape(-1)]})
    json.dump({"source": "reference " + steps_src + " and " + gauss_src, "steps": sw, "gaussian": gm},
              open(os.path.join(OUT, "sw_steps.json"), "w"))

    # ---- patch sampler (base_data_loader.py:64-139): get_bbox on a stub loader, numpy global RNG seeded per case
    bbox, bbox_src = ref_function("training/dataloading/base_data_loader.py", "get_bbox", "nnUNetDataLoaderBase",
                                  print=lambda *a, **k: None)
    rng = np.random.default_rng(11)
    out = []

    def locs(shape, n):
        if n == 0:
            return np.zeros((0, 4), dtype=np.int64)
        return np.stack([np.zeros(n, dtype=np.int64)] + [rng.integers(0, s, n) for s in shape], 1)

    scen = []
    for shape, patch, pad_extra in (((40, 50, 60), (32, 32, 32), (0, 0, 0)), ((20, 70, 33), (32, 48, 32), (0, 0, 0)),
                                    ((30, 30, 30), (32, 32, 32), (0, 0, 0)), ((64, 64, 64), (32, 40, 48), (5, 4, 3)),
                                    ((17, 90, 41), (16, 64, 48), (0, 7, 0))):
        for force_fg in (False, True):
            for variant in ("plain", "empty_class", "all_empty", "overwrite", "region_key", "ignore"):
                scen.append((shape, patch, pad_extra, force_fg, variant))
    for ci, (shape, patch, pad_extra, force_fg, variant) in enumerate(scen):
        all_labels = (1, 2, 3)
        cl = {1: locs(shape, 40), 2: locs(shape, 25), 3: locs(shape, 7)}
        overwrite, has_ignore = None, False
        if variant == "empty_class":
            cl[2] = locs(shape, 0)
        elif variant == "all_empty":
            cl = {k: locs(shape, 0) for k in cl}
        elif variant == "overwrite":
            overwrite = 3
        elif variant == "region_key":
            cl[all_labels] = locs(shape, 30)  # the annotated-classes tuple key (removed when other classes exist)
        elif variant == "ignore":
            has_ignore = True
            cl[all_labels] = locs(shape, 30 if ci % 2 else 0)
        me = types.SimpleNamespace(need_to_pad=np.array(pad_extra, dtype=int), patch_size=patch,
                                   has_ignore=has_ignore, annotated_classes_key=all_labels)
        seed = 1000 + ci
        np.random.seed(seed)
        lbs, ubs = bbox(me, np.array(shape), force_fg, cl, overwrite)
        tail = float(np.random.uniform())  # the RNG state after the call: pins the NUMBER and ORDER of draws
        out.append({"shape": list(shape), "patch_size": list(patch), "need_to_pad": list(pad_extra),
                    "force_fg": force_fg, "has_ignore": has_ignore, "overwrite_class": overwrite, "seed": seed,
                    "annotated_classes_key": list(all_labels),
                    "class_locations": [[(list(k) if isinstance(k, tuple) else k), v.tolist()] for k, v in cl.items()],
                    "bbox_lbs": [int(v) for v in lbs], "bbox_ubs": [int(v) for v in ubs], "rng_tail": tail})
    json.dump({"source": "reference " + bbox_src + " (method executed on a stub loader)", "cases": out},
              open(os.path.join(OUT, "get_bbox.json"), "w"))
    print("wrote distill_kl_* feat_kl_* l2_loss_plain ddp_split.json sw_steps.json get_bbox.json (reference-extracted)")


# ------------------------------------------------------------------ oracle-generated (reference not importable)
def loss_fixtures():
    # DC+CE on one level, batch_dice False/True
    for bd in (False, True):
        g = gen(53)
        logits = (torch.randn(2, 5, 8, 8, 8, generator=g) * 2).requires_grad_()
        tgt = torch.round(torch.rand(2, 1, 8, 8, 8, generator=g) * 4)
        lf = LO.build_loss(1, batch_dice=bd, deep_supervision=False)
        l = lf(logits, tgt)
        l.backward()
        tp, fp, fn = LO.validation_counts(logits.detach(), tgt)
        per, mean = LO.dice_from_counts(tp, fp, fn)
        save(f"dc_ce_batchdice{int(bd)}.npz", source="oracle restatement (App. B; nnUNetTrainer.py:351-375)",
             logits=logits, target=tgt, loss=l, glogits=logits.grad, tp=tp, fp=fp, fn=fn, dice_per_class=per,
             dice_mean=mean)
    # soft clDice
    g = gen(54)
    p = torch.rand(2, 1, 10, 12, 9, generator=g).requires_grad_()
    t = (F.avg_pool3d(torch.rand(2, 1, 10, 12, 9, generator=g), 3, 1, 1) > 0.5).float()
    l = LO.soft_cldice(p, t, 3, 1.0)
    l.backward()
    save("soft_cldice.npz", source="oracle (reference soft_skel + clDice_metric.py:7-36 formula)", iter=3, smooth=1.0,
         pred=p, target=t, loss=l, gpred=p.grad)


class _RefStepHarness:
    """The reference's own step code on a stub trainer (nothing of its text is stored; see ref_function):
    * `nnUNetTrainer.train_step` (nnUNetTrainer.py:888-925) -- executed unchanged with `autocast` / `dummy_context`
      injected (the device is cpu, so the reference takes its dummy_context branch) and its debug prints muted;
    * `nnUNetTrainer.configure_optimizers` (:473-477) -- executed unchanged; `PolyLRScheduler` is a shim whose `step`
      is the reference's own `PolyLRScheduler.step` (polylr.py:13-20; the ctor passes a `verbose` positional that
      torch 2.10's LRScheduler no longer takes, an ordinary TypeError);
    * `nnUNetTrainer._get_deep_supervision_scales` (:296-302);
    * `UNetDecoder_return_last_fea.forward` (UNetDecoder.py:1001-1027) -- the fork's plain decoder forward (no
      attention insert, `attn_skip = skips[-1]`), executed with `self` = the oracle decoder module, which holds the
      `stages / transpconvs / seg_layers / deep_supervision` attributes the body reads.
    The encoder blocks, the loss classes and the MVD composite stay the oracle's restatement (un-vendored
    `dynamic_network_architectures`, three loss files missing from the fork: SURVEY 8c)."""
    TR = "training/nnUNetTrainer/nnUNetTrainer.py"

    def __init__(self):
        import contextlib
        import types
        quiet = lambda *a, **k: None
        self.types = types
        self.train_step, self.src_step = ref_function(self.TR, "train_step", "nnUNetTrainer", autocast=torch.autocast,
                                                      dummy_context=contextlib.nullcontext, print=quiet)
        poly = ref_module("training/lr_scheduler/polylr.py", "ref_poly_step")

        class PolyShim:
            def __init__(sh, optimizer, initial_lr, max_steps, exponent=0.9, current_step=None):
                sh.optimizer, sh.initial_lr, sh.max_steps, sh.exponent, sh.ctr = optimizer, initial_lr, max_steps, exponent, 0
            step = poly.PolyLRScheduler.step

        self.configure_optimizers, self.src_opt = ref_function(self.TR, "configure_optimizers", "nnUNetTrainer",
                                                               PolyLRScheduler=PolyShim)
        self.ds_scales, self.src_ds = ref_function(self.TR, "_get_deep_supervision_scales", "nnUNetTrainer")
        self.dec_forward, self.src_dec = ref_function("training/my_network/UNetDecoder.py", "forward",
                                                      "UNetDecoder_return_last_fea", print=quiet)

    def network(self, net):
        """encoder (oracle) -> the reference's decoder forward.  Returns a callable with the `parameters()` the trainer
        methods use and a `.last` slot holding the outputs of the latest call."""
        h = self

        class Net:
            last = None

            def __call__(s, x):
                skips = net.encoder(x)
                r = h.dec_forward(net.decoder, skips, skips[-1])
                s.last = r
                return r[0] if net.decoder.deep_supervision else r

            def parameters(s):
                return net.parameters()
        return Net()

    def trainer(self, net, loss_fn, num_epochs=200):
        me = self.types.SimpleNamespace(network=self.network(net), loss=loss_fn, device=torch.device("cpu"),
                                        grad_scaler=None, initial_lr=1e-2, weight_decay=3e-5, num_epochs=num_epochs)
        me.optimizer, me.lr_scheduler = self.configure_optimizers(me)
        return me

    def scales(self, strides, enabled=True):
        me = self.types.SimpleNamespace(enable_deep_supervision=enabled,
                                        configuration_manager=self.types.SimpleNamespace(pool_op_kernel_sizes=strides))
        return self.ds_scales(me)


def _assert_same_state(net_a, net_b, what):
    for (n, a), (_, b) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), (what, n)
        if a.grad is not None or b.grad is not None:
            assert torch.equal(a.grad, b.grad), (what, "grad", n)


def ds_scales_fixture(H):
    cases = []
    for strides in ([[1, 1, 1]] + [[2, 2, 2]] * 5, [[1, 1, 1]] + [[2, 2, 2]] * 4, [[1, 1, 1], [2, 2, 2], [2, 2, 2]],
                    [[1, 1, 1], [1, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2]], [[1, 1, 1]]):
        sc = H.scales(strides)
        assert [list(map(float, i)) for i in sc] == [list(map(float, i)) for i in SO.ds_scales(strides)]
        cases.append({"pool_op_kernel_sizes": strides, "scales": [[float(v) for v in i] for i in sc]})
    assert H.scales([[1, 1, 1], [2, 2, 2]], enabled=False) is None
    # configure_optimizers (:473-477) on a stub trainer: the SGD hyper-parameters and the schedule it attaches
    me = H.types.SimpleNamespace(network=torch.nn.Linear(2, 2), initial_lr=1e-2, weight_decay=3e-5, num_epochs=50)
    opt, sch = H.configure_optimizers(me)
    g0 = opt.param_groups[0]
    hp = {k: g0[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")}
    lrs = []
    for e in range(50):
        sch.step(e)
        lrs.append(opt.param_groups[0]['lr'])
    json.dump({"source": "reference " + H.src_ds + " and " + H.src_opt + " (methods executed on a stub trainer)",
               "cases": cases, "disabled": None,
               "optimizer": {"class": type(opt).__name__, "hyper": hp, "num_epochs": 50, "lrs": lrs}},
              open(os.path.join(OUT, "ds_scales.json"), "w"))
    print("wrote ds_scales.json")


def unet_step_fixture():
    """Tiny end-to-end: 3 stages [8,16,32], C_in=2, K=3, 16^3, B=2 (App. E `unet_tiny_step`).  Round 3: the three steps
    are run by the REFERENCE's train_step / configure_optimizers / decoder forward (_RefStepHarness); the oracle
    restatement runs beside it on a copy of the network and must agree bit for bit at every step."""
    import copy
    H = _RefStepHarness()
    ds_scales_fixture(H)
    strides = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
    net = UO.build_plainconv_unet(2, 3, 3, strides, features_per_stage=[8, 16, 32], seed=0)
    # non-trivial norm affine + biases so that every parameter's gradient is exercised
    g = gen(60)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    batch = SO.synthetic_batch(2, 2, (16, 16, 16), strides, num_classes=3, seed=1234)
    loss_fn = LO.build_loss(len(batch['target']))
    twin = copy.deepcopy(net)                       # the oracle restatement, same start
    opt_twin = SO.make_optimizer(twin.parameters())
    me = H.trainer(net, loss_fn)
    g0 = me.optimizer.param_groups[0]
    assert isinstance(me.optimizer, torch.optim.SGD) and (g0['lr'], g0['momentum'], g0['weight_decay'], g0['nesterov']) == \
        (1e-2, 0.99, 3e-5, True)
    out = {"source": f"reference {H.src_step}, {H.src_opt} (methods executed on a stub trainer; cpu branch), network = "
                     f"oracle encoder blocks + reference {H.src_dec}; loss = oracle restatement (App. B)",
           "strides": strides, "features": [8, 16, 32], "num_classes": 3, "data": batch['data']}
    for i, t in enumerate(batch['target']):
        out[f"target{i}"] = t
    for k, v in sd0.items():
        out["sd0/" + k] = v
    for step in range(3):
        r = H.train_step(me, batch)
        l, (logits, feat) = r['loss'], me.network.last
        lo, logits_o, gn = SO.train_step(twin, loss_fn, opt_twin, batch)
        assert l.dtype == np.float32 and np.array_equal(l, lo), (step, l, lo)
        assert all(torch.equal(a, b) for a, b in zip(logits, logits_o))
        _assert_same_state(net, twin, f"step {step}")
        out[f"loss{step}"] = l
        out[f"gradnorm{step}"] = gn   # norm before clipping (the reference drops clip_grad_norm_'s return value; the
        #                               twin's post-clip gradients equal the reference's, asserted above)
        if step == 0:
            for i, lg in enumerate(logits):
                out[f"logits{i}"] = lg.detach()
            out["feat"] = feat.detach()
            for n, p in net.named_parameters():
                out["grad0/" + n] = p.grad.clone()
        for n, p in net.named_parameters():
            if step in (0, 2):
                out[f"sd{step + 1}/" + n] = p.detach().clone()
    tp, fp, fn = LO.validation_counts(net(batch['data'])[0].detach(), batch['target'][0])
    out["val_tp"], out["val_fp"], out["val_fn"] = tp, fp, fn
    save("unet_tiny_step.npz", **out)

    # the decoder forward alone: DS on (list + last feature) and DS off (bare tensor), reference vs restatement
    with torch.no_grad():
        skips = net.encoder(batch['data'])
        r_on = H.dec_forward(net.decoder, skips, skips[-1])
        o_on = net.decoder(skips, True)
        assert all(torch.equal(a, b) for a, b in zip(r_on[0], o_on[0])) and torch.equal(r_on[1], o_on[1])
        net.decoder.deep_supervision = False
        r_off = H.dec_forward(net.decoder, skips, skips[-1])
        o_off = net.decoder(skips)
        net.decoder.deep_supervision = True
        assert torch.is_tensor(r_off) and torch.equal(r_off, o_off) and torch.equal(r_off, r_on[0][0])
    dec = {"source": "reference " + H.src_dec + " (executed with self = the oracle decoder module)",
           "strides": strides, "features": [8, 16, 32], "num_classes": 3, "feat": r_on[1], "logits_ds_off": r_off}
    for i, sk in enumerate(skips):
        dec[f"skip{i}"] = sk
    for i, lg in enumerate(r_on[0]):
        dec[f"logits{i}"] = lg
    for k, v in net.decoder.state_dict().items():
        if not k.startswith("encoder."):
            dec["sd/" + k] = v
    save("decoder_forward.npz", **dec)

    # anisotropic / no-DS variant: strides (1,2,2) then (2,2,2); checks per-axis stride handling
    strides = [[1, 1, 1], [1, 2, 2], [2, 2, 2]]
    net = UO.build_plainconv_unet(1, 2, 3, strides, features_per_stage=[4, 8, 16], seed=1)
    g = gen(61)
    data = torch.rand(1, 1, 8, 16, 12, generator=g)
    outs = H.network(net)(data)
    assert all(torch.equal(a, b) for a, b in zip(outs, net(data)))
    o = {"source": "oracle encoder blocks + reference " + H.src_dec, "strides": strides, "features": [4, 8, 16],
         "num_classes": 2, "data": data}
    for k, v in net.state_dict().items():
        o["sd0/" + k] = v
    for i, lg in enumerate(outs):
        o[f"logits{i}"] = lg.detach()
    save("unet_aniso_fwd.npz", **o)


def mvd_step_fixture():
    """Dual-branch step.  The composite loss is the build's restatement (MVDTrainer.py:879-925 is not executable: undefined
    names); each branch's decoder runs through the REFERENCE's UNetDecoder_return_last_fea.forward, the
    optimizer comes from the reference's configure_optimizers, and a twin on the oracle's own decoder must agree exactly."""
    import copy
    H = _RefStepHarness()
    strides = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
    n1 = UO.build_plainconv_unet(2, 4, 3, strides, features_per_stage=[8, 16, 32], seed=2)
    n2 = UO.build_plainconv_unet(2, 4, 3, strides, features_per_stage=[8, 16, 32], seed=3)
    net = UO.DualBranchNet(n1, n2)
    twin = copy.deepcopy(net)
    batch = SO.synthetic_batch(2, 2, (16, 16, 16), strides, num_classes=4, seed=77)
    loss_fn = LO.build_loss(len(batch['target']))

    class RefDecoders:
        """(logits_1, logits_2, feat_1, feat_2) with both decoders run by the reference's forward."""
        def __call__(s, x):
            sk1, sk2 = n1.encoder(x), n2.encoder(x)
            r1, r2 = H.dec_forward(n1.decoder, sk1, sk1[-1]), H.dec_forward(n2.decoder, sk2, sk2[-1])
            return r1[0], r2[0], r1[1], r2[1]

        def parameters(s):
            return net.parameters()

    me = H.types.SimpleNamespace(network=net, initial_lr=1e-2, weight_decay=3e-5, num_epochs=200)
    opt, _sch = H.configure_optimizers(me)
    opt_twin = SO.make_optimizer(twin.parameters())
    out = {"source": "oracle restatement of MVDTrainer.py:879-925 (see oracle/step_oracle.py); decoders run by reference "
                     + H.src_dec + ", optimizer from reference " + H.src_opt, "strides": strides,
           "features": [8, 16, 32], "num_classes": 4, "data": batch['data'], "skel_iter": 3}
    for i, t in enumerate(batch['target']):
        out[f"target{i}"] = t
    for k, v in net.state_dict().items():
        out["sd0/" + k] = v.clone()
    l, outs, gn = SO.mvd_train_step(RefDecoders(), loss_fn, opt, batch, use_topo=True, skel_iter=3, feat_kl=True)
    lt, _o, gnt = SO.mvd_train_step(twin, loss_fn, opt_twin, batch, use_topo=True, skel_iter=3, feat_kl=True)
    assert np.array_equal(l, lt) and gn == gnt
    _assert_same_state(net, twin, "mvd step")
    out["loss0"], out["gradnorm0"] = l, gn
    for n, p in net.named_parameters():
        out["grad0/" + n] = p.grad.clone()
        out["sd1/" + n] = p.detach().clone()
    save("mvd_tiny_step.npz", **out)


def persistence_fixtures():
    m = build_ref.load()
    assert m is not None, "run `python oracle/build_ref.py` first"
    srt = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]
    cases = []
    rng = np.random.default_rng(7)

    def run_ref(cells, f, maxdim=0):
        s = m.SimplicialComplex()
        for c in cells:
            s.append(list(c))
        s.initialize()
        s.extendFloat(torch.from_numpy(f.reshape(-1).copy()))
        hom = m.persistenceForwardHom(s, maxdim, 0)[0].detach().numpy().copy()
        s2 = m.SimplicialComplex()
        for c in cells:
            s2.append(list(c))
        s2.initialize()
        s2.extendFloat(torch.from_numpy(f.reshape(-1).copy()))
        coh = m.persistenceForwardCohom(s2, maxdim)[0].detach().numpy().copy()
        assert np.array_equal(srt(hom), srt(coh))
        return srt(hom)

    def grid_cells(D, H, W, conn):
        cells = [[i] for i in range(D * H * W)]
        offs = {6: [(0, 0, 1), (0, 1, 0), (1, 0, 0)],
                14: [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)]}[conn]
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    for dz, dy, dx in offs:
                        zz, yy, xx = z + dz, y + dy, x + dx
                        if zz < D and yy < H and xx < W:
                            cells.append([(z * H + y) * W + x, (zz * H + yy) * W + xx])
        return cells

    for (D, H, W), conn, ties in (((1, 1, 5), 6, False), ((1, 1, 64), 6, False), ((1, 4, 4), 14, False),
                                  ((1, 8, 8), 14, True), ((1, 16, 16), 14, False), ((4, 4, 4), 6, False),
                                  ((5, 6, 7), 6, True), ((4, 5, 6), 14, False), ((6, 6, 6), 6, False)):
        f = rng.random((D, H, W)).astype(np.float32)
        if ties:
            f = np.round(f * 4) / 4
        dgm = run_ref(grid_cells(D, H, W, conn), f)
        b, d, _ = cc_oracle.h0_persistence(f, conn)
        assert np.array_equal(dgm, srt(np.stack([b, d], 1))), "C oracle differs from the reference C++"
        cases.append({"shape": [D, H, W], "conn": conn, "f": f.reshape(-1).tolist(),
                      "dgm0_sorted": [[float(a), (None if np.isinf(c) else float(c))] for a, c in dgm]})
    # the survey's 5-vertex line known answer
    f = np.array([0.0, 3.0, 0.5, 2.0, 1.0], dtype=np.float32).reshape(1, 1, 5)
    dgm = run_ref(grid_cells(1, 1, 5, 6), f)
    cases.append({"shape": [1, 1, 5], "conn": 6, "f": f.reshape(-1).tolist(),
                  "dgm0_sorted": [[float(a), (None if np.isinf(c) else float(c))] for a, c in dgm]})
    json.dump({"source": "reference C++ persistence (hom.cpp + cohom.cpp) compiled into oracle/_ref", "cases": cases},
              open(os.path.join(OUT, "persistence_grid.json"), "w"))
    # connected components: #infinite H0 bars of the thresholded mask == CC count (reference-pinned count)
    cc_cases = []
    for (D, H, W), conn in (((6, 7, 8), 6), ((5, 5, 5), 14), ((1, 12, 12), 6)):
        mask = (rng.random((D, H, W)) > 0.55)
        labels, n = cc_oracle.cc_label(mask, conn)
        # reference: sub-complex on mask vertices -> count essential bars
        idx = -np.ones(mask.size, dtype=np.int64)
        idx[mask.reshape(-1)] = np.arange(mask.sum())
        cells = [c for c in grid_cells(D, H, W, conn) if all(mask.reshape(-1)[v] for v in c)]
        cells = [[int(idx[v]) for v in c] for c in cells]
        dgm = run_ref(cells, np.zeros(int(mask.sum()), dtype=np.float32))
        assert int(np.isinf(dgm[:, 1]).sum()) == n
        cc_cases.append({"shape": [D, H, W], "conn": conn, "mask": mask.reshape(-1).astype(int).tolist(),
                         "labels": labels.reshape(-1).tolist(), "count": n})
    json.dump({"source": "labels: oracle/cc_oracle.c (canonical = 1 + min linear index); count cross-checked "
                         "against the reference C++ (essential H0 bars)", "cases": cc_cases},
              open(os.path.join(OUT, "cc_label.json"), "w"))
    print("wrote persistence_grid.json cc_label.json")


# ------------------------------------------------------------------ the cases tests/test_oracle.py once ran the reference on
def oracle_check_fixtures():
    """Inputs and outputs of three reference modules (soft_skeleton, robust_ce_loss, network_initialization) and of the
    reference's C++ persistence extension, on the small cases tests/test_oracle.py pins the oracle to."""
    g = gen(5)
    x = torch.rand(1, 2, 9, 8, 7, generator=g)
    sk = ref_module("training/loss/soft_skeleton.py", "ref_skel_live")
    skel = {f"skel_iter{it}": sk.soft_skel(x, it) for it in (0, 2, 5)}
    rce = ref_module("training/loss/robust_ce_loss.py", "ref_rce_live")
    logits = torch.randn(2, 4, 3, 3, 3, generator=g)
    tgt = torch.round(torch.rand(2, 1, 3, 3, 3, generator=g) * 3)
    loss = rce.RobustCrossEntropyLoss()(logits, tgt)
    init = ref_module("utilities/network_initialization.py", "ref_init_live")
    torch.manual_seed(11)
    conv = torch.nn.Conv3d(4, 8, 3)
    conv.apply(init.InitWeights_He(1e-2))
    save("reference_modules.npz", source="reference soft_skeleton.py:6-37, robust_ce_loss.py:6-16, "
                                         "network_initialization.py:4-12", x=x, logits=logits, target=tgt, ce_loss=loss,
         he_seed=11, he_weight=conv.weight, **skel)

    m = build_ref.load()
    assert m is not None, "run `python oracle/build_ref.py` first"
    rng = np.random.default_rng(9)
    D, H, W = 3, 4, 5
    f = (np.round(rng.random((D, H, W)) * 8) / 8).astype(np.float32)  # ties on purpose
    s = m.SimplicialComplex()
    for i in range(D * H * W):
        s.append([i])
    for z in range(D):
        for y in range(H):
            for x in range(W):
                for dz, dy, dx in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
                    if z + dz < D and y + dy < H and x + dx < W:
                        s.append([(z * H + y) * W + x, ((z + dz) * H + y + dy) * W + x + dx])
    s.initialize()
    s.extendFloat(torch.from_numpy(f.reshape(-1).copy()))
    save("ref_persistence_3x4x5.npz", source="reference C++ persistence (hom.cpp) compiled into oracle/_ref", f=f,
         dgm0=m.persistenceForwardHom(s, 0, 0)[0])


# ------------------------------------------------------------------ regions / ignore label
def region_label_fixtures():
    """tests/golden/label_manager.json: the reference's own LabelManager (label_handling.py) and
    ConvertSegmentationToRegionsTransform (region_based_training.py) -- both need only numpy and torch once
    AbstractTransform, bounding_box_to_slice and softmax_helper_dim0 are stubbed -- executed on small inputs."""
    LM, lm_src = ref_function("utilities/label_handling/label_handling.py", "LabelManager",
                              softmax_helper_dim0=lambda x: torch.softmax(x, 0),
                              bounding_box_to_slice=lambda bb: tuple(slice(*i) for i in bb))
    TR, tr_src = ref_function("training/data_augmentation/custom_transforms/region_based_training.py",
                              "ConvertSegmentationToRegionsTransform", AbstractTransform=object)

    def plain(v):
        if isinstance(v, (list, tuple)):
            return [plain(i) for i in v]
        return int(v) if isinstance(v, (int, np.integer)) else v

    dicts = [
        ({"background": 0, "a": 1, "b": 2}, None),
        ({"background": 0, "a": 1}, None),
        ({"background": 0, "a": 1, "b": 2, "c": 3, "d": 4}, None),
        ({"background": 0, "a": 1, "b": 2, "ignore": 3}, None),
        ({"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, [1, 2, 3]),
        ({"background": 0, "whole": (1, 2, 3), "core": (2, 3), "enh": 3}, [1, 2, 3]),
        ({"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3, "ignore": 4}, [1, 2, 3]),
        ({"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, [3, 1, 2]),
        ({"background": 0, "with_bg": [0, 1], "b": 2}, [1, 2]),
        ({"background": 0, "zeros": [0, 0], "ab": [1, 2], "b": 2}, [1, 2]),
        ({"background": 0, "single": [1], "pair": (1, 2)}, [2, 1]),
        ({"background": 0, "a": 1, "bc": [2, 3], "c": 3, "d": [4], "ignore": 5}, [1, 2, 3, 4]),
    ]
    managers = []
    for d, order in dicts:
        m = LM(d, order)
        managers.append({"label_dict": plain({k: v for k, v in d.items()}),
                         "is_tuple": {k: isinstance(v, tuple) for k, v in d.items()},
                         "regions_class_order": order, "has_regions": bool(m.has_regions),
                         "has_ignore_label": bool(m.has_ignore_label), "ignore_label": m.ignore_label,
                         "all_labels": plain(m.all_labels),
                         "all_regions": None if m.all_regions is None else plain(m.all_regions),
                         "foreground_regions": plain(m.foreground_regions) if m.has_regions else None,
                         "foreground_labels": plain(m.foreground_labels),
                         "num_segmentation_heads": int(m.num_segmentation_heads)})
    rejected = []
    for d, order in (({"background": 0, "a": 1, "ignore": 3}, None), ({"background": 0, "a": 1, "b": 2, "ignore": 1}, None),
                     ({"a": 1}, None), ({"background": [0, 1], "a": 2}, None), ({"background": 0, "r": [1, 2]}, None),
                     ({"background": 0, "r": [1, 2], "s": 2}, [1])):
        try:
            LM(d, order)
            raise SystemExit(f"the reference accepted {d}")
        except (AssertionError, RuntimeError) as e:
            rejected.append({"label_dict": plain(d), "regions_class_order": order, "error": type(e).__name__})
    rng = np.random.RandomState(17)
    conv = []
    d3 = {"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}
    for order in ([1, 2, 3], [3, 2, 1], [2, 3, 1], [1, 3, 2], [7, 5, 9]):
        m = LM(d3, order)
        p = rng.rand(3, 4, 5, 6).astype(np.float32)
        p.flat[rng.choice(p.size, 12, replace=False)] = 0.5   # exactly 0.5 is "off"
        conv.append({"regions_class_order": order, "probabilities": p.tolist(),
                     "segmentation": m.convert_probabilities_to_segmentation(p).astype(np.int64).tolist()})
    planes = []
    for regions, ign, nlab in ((d3, None, 4), (d3, 4, 5), ({"background": 0, "with_bg": [0, 1], "b": 2}, None, 3),
                               ({"background": 0, "a": 1, "bc": [2, 3], "c": 3, "d": [4]}, 5, 6)):
        m = LM(dict(regions, **({"ignore": ign} if ign is not None else {})), list(range(1, len(regions))))
        seg = rng.randint(0, nlab, size=(2, 1, 3, 4, 5)).astype(np.float32)
        regs = list(m.foreground_regions) + [ign] if ign is not None else m.foreground_regions   # nnUNetTrainer.py:759-763
        out = TR(regs, 'target', 'target')(target=seg)['target']
        planes.append({"foreground_regions": plain(m.foreground_regions), "ignore_label": ign, "seg": seg.tolist(),
                       "planes": out.tolist()})
    json.dump({"source": f"reference {lm_src} and {tr_src} (classes executed with AbstractTransform, "
                         f"bounding_box_to_slice and softmax_helper_dim0 stubbed)",
               "managers": managers, "rejected": rejected, "convert_probabilities_to_segmentation": conv,
               "regions_transform": planes}, open(os.path.join(OUT, "label_manager.json"), "w"))
    print("wrote label_manager.json")


# ------------------------------------------------------------------ 2-D training loader (data_loader_2d.py:7-86)
def loader2d_fixture():
    """tests/golden/loader2d.json: the reference's own nnUNetDataLoader2D.generate_train_batch and get_bbox bodies executed
    on a stub loader over toy cases (numpy global RNG seeded per scenario).  Per batch: keys, the slice and box of every
    sample, and one uniform drawn after the batch (pins the number and order of draws).  The slice is read back from the
    returned data (channel 0 of a toy case holds z + 1), the box from the get_bbox call.  Data only; cases are stored as
    shape + class_locations."""
    import types
    gtb, src1 = ref_function("training/dataloading/data_loader_2d.py", "generate_train_batch", "nnUNetDataLoader2D")
    bbox, src2 = ref_function("training/dataloading/base_data_loader.py", "get_bbox", "nnUNetDataLoaderBase",
                              print=lambda *a, **k: None)
    rng = np.random.default_rng(23)
    labels = (1, 2)

    def locs(shape, n):
        if n == 0:
            return np.zeros((0, 4), dtype=np.int64)
        return np.stack([np.zeros(n, dtype=np.int64)] + [rng.integers(0, s, n) for s in shape], 1)

    scenarios = []
    for name, has_ignore in (("plain", False), ("ignore", True)):
        cases = {}
        # a case larger than the patch, one smaller than it in both axes, one smaller in one axis, one without foreground
        for key, shape, n1, n2 in (("a", (6, 48, 60), 30, 12), ("b", (5, 20, 30), 15, 0), ("c", (7, 64, 36), 20, 9),
                                   ("d", (4, 50, 50), 0, 0)):
            cl = {1: locs(shape, n1), 2: locs(shape, n2)}
            if has_ignore:
                cl[labels] = locs(shape, 25)   # the annotated-classes key: every case has annotated voxels
            cases[key] = (shape, cl)
        scenarios.append((name, has_ignore, cases))
    out = []
    for si, (name, has_ignore, cases) in enumerate(scenarios):
        patch, final, bs, C = (40, 44), (32, 40), 6, 2
        boxes = []

        def load_case(key, cases=cases):
            shape, cl = cases[key]
            data = np.zeros((C, *shape), dtype=np.float32)
            data[0] = (np.arange(shape[0], dtype=np.float32) + 1)[:, None, None]
            return data, np.zeros((1, *shape), dtype=np.int16), {"class_locations": cl}

        me = types.SimpleNamespace(
            need_to_pad=(np.array(patch) - np.array(final)).astype(int), patch_size=patch, has_ignore=has_ignore,
            annotated_classes_key=labels, data_shape=(bs, C, *patch), seg_shape=(bs, 1, *patch),
            _data=types.SimpleNamespace(load_case=load_case),
            get_indices=lambda cases=cases: np.random.choice(list(cases.keys()), bs, True, None),
            get_do_oversample=lambda j: not j < round(bs * (1 - 0.33)))

        def get_bbox(*a, **k):
            r = bbox(me, *a, **k)
            boxes.append(([int(v) for v in r[0]], [int(v) for v in r[1]]))
            return r
        me.get_bbox = get_bbox
        seed = 500 + si
        np.random.seed(seed)
        batches = []
        for _ in range(6):
            del boxes[:]
            b = gtb(me)
            slices = [int(round(float(b["data"][j, 0].max()))) - 1 for j in range(bs)]
            batches.append({"keys": [str(k) for k in b["keys"]], "slices": slices, "bbox_lbs": [x[0] for x in boxes],
                            "bbox_ubs": [x[1] for x in boxes], "rng_tail": float(np.random.uniform())})
        out.append({"name": name, "has_ignore": has_ignore, "seed": seed, "batch_size": bs, "channels": C,
                    "patch_size": list(patch), "final_patch_size": list(final), "oversample_foreground_percent": 0.33,
                    "all_labels": list(labels),
                    "cases": {k: {"shape": list(sh), "class_locations": [[(list(c) if isinstance(c, tuple) else c), v.tolist()]
                                                                         for c, v in cl.items()]}
                              for k, (sh, cl) in cases.items()},
                    "batches": batches})
    json.dump({"source": "reference " + src1 + " and " + src2 + " (method bodies executed on a stub loader)",
               "scenarios": out}, open(os.path.join(OUT, "loader2d.json"), "w"))
    print("wrote loader2d.json")


# ------------------------------------------------------------------ Cross_Attention / Self_Attention (UNetDecoder.py:1087-1154)
def cross_attention_fixture():
    """The reference's own attention class bodies (they need only torch), eval mode, fp64, B = 2, N = 16, C = 32, 8 heads,
    random weights.  Self_Attention is run twice, the second time with another `proj`: its output ignores proj
    (UNetDecoder.py:1151-1154 return the tensor before the projection)."""
    CA, ca_src = ref_function("training/my_network/UNetDecoder.py", "Cross_Attention", nn=torch.nn)
    SA, sa_src = ref_function("training/my_network/UNetDecoder.py", "Self_Attention", nn=torch.nn)
    B, N, C, H = 2, 16, 32, 8
    g = gen(20260)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ca = CA(dim=C, num_heads=H, qkv_bias=False, attn_drop=0.1, proj_drop=0.1).double().eval()
    sa = SA(dim=C, num_heads=H, qkv_bias=False, attn_drop=0.1, proj_drop=0.1).double().eval()
    with torch.no_grad():
        for p in list(ca.parameters()) + list(sa.parameters()):
            p.copy_(rnd(*p.shape) * 0.3)
        x1, x2 = rnd(B, N, C), rnd(B, N, C)
        o1, o2 = ca(x1, x2)
        so = sa(x1)
        proj_w, proj_b = sa.proj.weight.clone(), sa.proj.bias.clone()
        sa.proj.weight.copy_(rnd(C, C))
        sa.proj.bias.copy_(rnd(C))
        so_other_proj = sa(x1)
    arrs = {"ca/" + k: v for k, v in ca.state_dict().items()}
    arrs.update({"sa/qkv.weight": sa.qkv.weight, "sa/proj.weight": proj_w, "sa/proj.bias": proj_b,
                 "sa/proj2.weight": sa.proj.weight, "sa/proj2.bias": sa.proj.bias})
    save("cross_attention.npz", x1=x1, x2=x2, ca_out1=o1, ca_out2=o2, sa_out=so, sa_out_other_proj=so_other_proj,
         heads=np.int64(H), source=np.array(f"reference {ca_src}, {sa_src}"), **arrs)


# ------------------------------------------------------------------ TopKLoss (training/loss/robust_ce_loss.py:19-32)
TOPK_CASES = [
    # name, N, K, spatial, kwargs of TopKLoss, ignored fraction (of the voxels, relabelled `ignore_index`), logit scale
    ("plain_n1_k2", 1, 2, (5, 7, 9), {}, 0.0, 2.0),
    ("smooth_n3_k3", 3, 3, (5, 7, 9), {"label_smoothing": 0.1}, 0.0, 2.0),
    ("ignore_few_n1_k5", 1, 5, (5, 7, 9), {"ignore_index": 5}, 0.05, 2.0),
    ("plain_n3_k8", 3, 8, (5, 7, 9), {}, 0.0, 2.0),
    ("ignore_most_n1_k3", 1, 3, (5, 7, 9), {"ignore_index": 3}, 0.95, 2.0),
    ("ignore_smooth_n1_k5", 1, 5, (5, 7, 9), {"ignore_index": 5, "label_smoothing": 0.1}, 0.3, 2.0),
    ("k_is_1", 1, 2, (2, 2, 3), {}, 0.0, 2.0),
    ("scaled40_n1_k3", 1, 3, (5, 7, 9), {}, 0.0, 80.0),
]


def topk_loss_fixture():
    """The reference's own TopKLoss class, executed in fp64 on the small cases of tests/test_gpu_topk.py: inputs, loss and
    dlogits per case, and the 'mostly ignored' case of DESIGN 29 (2 x 3 x 4^3, three valid voxels, k = 12).  No tie with a
    non-zero gradient occurs in these cases (torch.topk's choice among ties is unspecified), which the generator asserts."""
    m = ref_module("training/loss/robust_ce_loss.py", "ref_robust_ce_loss")
    arrs, names = {}, []
    cases = list(TOPK_CASES) + [("mostly_ignored", 2, 3, (4, 4, 4), {"ignore_index": 3}, None, 2.0)]
    for ci, (name, N, K, sp, kw, frac, scale) in enumerate(cases):
        g = gen(29000 + ci)
        z32 = (torch.randn((N, K, *sp), generator=g) * scale).float()
        t = torch.randint(0, K, (N, 1, *sp), generator=g).float()
        ign = kw.get("ignore_index", -100)
        if frac is None:            # all but three voxels ignored
            keep = torch.randperm(t.numel(), generator=g)[:3]
            flat = torch.full((t.numel(),), float(ign))
            flat[keep] = t.reshape(-1)[keep]
            t = flat.reshape(t.shape)
        elif frac > 0:
            t[torch.rand(t.shape, generator=g) < frac] = float(ign)
        z = z32.double().requires_grad_(True)
        loss = m.TopKLoss(**kw)(z, t)
        loss.backward()
        with torch.no_grad():
            ce = F.cross_entropy(z, t[:, 0].long(), ignore_index=ign, reduction='none',
                                 label_smoothing=kw.get("label_smoothing", 0)).reshape(-1)
            k = int(np.int64(ce.numel()) * 10 / 100)
            thr = torch.sort(ce, descending=True).values[k - 1]
            assert float(thr) == 0.0 or int((ce == thr).sum()) == 1, name   # ties only among zeros (zero gradient)
        names.append(name)
        arrs[f"{name}/logits"] = z32
        arrs[f"{name}/target"] = t
        arrs[f"{name}/loss"] = loss.detach()
        arrs[f"{name}/dlogits"] = z.grad
        arrs[f"{name}/ignore_index"] = np.int64(ign)
        arrs[f"{name}/label_smoothing"] = np.float64(kw.get("label_smoothing", 0))
        arrs[f"{name}/k"] = np.int64(k)
    # k == 0: the reference's own answer, NaN (n = 8 voxels)
    z0 = torch.randn((1, 2, 2, 2, 2), generator=gen(29100), dtype=torch.float64)
    nan_loss = m.TopKLoss()(z0, torch.zeros((1, 1, 2, 2, 2)))
    assert bool(torch.isnan(nan_loss))
    save("topk_loss.npz", cases=np.array(names), k_zero_is_nan=np.bool_(True),
         source=np.array("reference training/loss/robust_ce_loss.py TopKLoss, fp64"), **arrs)


# ------------------------------------------------------------------ cascade transforms
def cascade_fixture():
    """tests/golden/cascade_transforms.npz: the reference's own ApplyRandomBinaryOperatorTransform and
    RemoveRandomConnectedComponentFromOneHotEncodingTransform class bodies (cascade_transforms.py), executed over the
    stand-ins of tools/cascade_standins.py for their three absent imports, with the trainer's parameters
    (nnUNetTrainer.py:741-755) on seeded inputs: 1 modality + K = 3 one-hot channels of 12 x 14 x 16, batch 2.  Per seed one
    transform instance is called twice (the shuffled channel list persists).  np.random.shuffle / np.random.choice are
    wrapped to record the channel order after each shuffle and the ordinal of the removed component; the wrappers call
    the originals, so the stream is untouched."""
    import cascade_standins
    cascade_standins.install()
    CT = ref_module("training/data_augmentation/custom_transforms/cascade_transforms.py", "ref_cascade_transforms")
    K, shape, B = 3, (12, 14, 16), 2
    idx = list(range(-K, 0))

    def inputs(seed):
        rng = np.random.RandomState(1000 + seed)
        coarse = rng.randint(0, K + 1, size=(B, 4, 5, 6))
        lab = coarse.repeat(3, 1).repeat(3, 2).repeat(3, 3)[:, :shape[0], :shape[1], :shape[2]]
        data = np.zeros((B, 1 + K, *shape), dtype=np.float32)
        data[:, 0] = rng.randint(0, 7, size=(B, *shape))
        for k in range(K):
            data[:, 1 + k] = lab == k + 1
        return data

    orig_shuffle, orig_choice = np.random.shuffle, np.random.choice
    arrs, bin_seeds, rem_seeds = {}, [], []
    for seed in range(60):
        # binary operators: two calls of one instance
        orders = []

        def shuffle(x):
            orig_shuffle(x)
            orders.append(list(x))
        np.random.shuffle = shuffle
        try:
            np.random.seed(seed)
            tr = CT.ApplyRandomBinaryOperatorTransform(channel_idx=list(idx), p_per_sample=0.4, key="data",
                                                       strel_size=(1, 8), p_per_label=1)
            d0 = inputs(seed)
            d1 = tr(data=d0.copy())["data"]
            d2 = tr(data=d1.copy())["data"]
        finally:
            np.random.shuffle = orig_shuffle
        if len(bin_seeds) < 6 and (len(orders) >= 2 or (seed % 7 == 0 and len(orders) == 0)):
            bin_seeds.append(seed)
            arrs[f"bin{seed}_in"], arrs[f"bin{seed}_out1"], arrs[f"bin{seed}_out2"] = d0, d1, d2
            arrs[f"bin{seed}_orders"] = np.asarray(orders, dtype=np.int64).reshape(-1, K)
        # removal: one call; the first choice of each event is the component
        picks = []

        def choice(a, *args, **kw):
            r = orig_choice(a, *args, **kw)
            picks.append((list(a).index(r), len(a)))
            return r
        np.random.choice = choice
        try:
            np.random.seed(seed)
            tr = CT.RemoveRandomConnectedComponentFromOneHotEncodingTransform(
                channel_idx=list(idx), key="data", p_per_sample=0.2, fill_with_other_class_p=0,
                dont_do_if_covers_more_than_x_percent=0.15)
            r0 = inputs(seed)
            r1 = tr(data=r0.copy())["data"]
        finally:
            np.random.choice = orig_choice
        if len(rem_seeds) < 5 and picks:
            changed = [(b, c) for b in range(B) for c in range(1, 1 + K) if not np.array_equal(r0[b, c], r1[b, c])]
            assert len(changed) == len(picks), "every removal changes exactly its own channel"
            rem_seeds.append(seed)
            arrs[f"rem{seed}_in"], arrs[f"rem{seed}_out"] = r0, r1
            arrs[f"rem{seed}_events"] = np.asarray([(b, c - 1 - K, o, n) for (b, c), (o, n) in zip(changed, picks)],
                                                  dtype=np.int64)
    assert len(bin_seeds) == 6 and len(rem_seeds) == 5
    assert any(len(arrs[f"bin{s}_orders"]) == 0 for s in bin_seeds), "one seed where the operator never fires"
    save("cascade_transforms.npz", source=np.array(
        "reference training/data_augmentation/custom_transforms/cascade_transforms.py (class bodies executed over "
        "tools/cascade_standins.py), p_per_sample 0.4 / strel (1, 8) and 0.2 / fill 0 / 0.15"),
        bin_seeds=np.asarray(bin_seeds), rem_seeds=np.asarray(rem_seeds), channel_idx=np.asarray(idx), **arrs)


# ------------------------------------------------------------------ ensembling
def ensemble_fixture():
    """tests/golden/ensemble.npz: the reference's own average_probabilities body (ensembling/ensemble.py) run on temporary
    .npz files of M = 3 softmax volumes [3, 6, 7, 9], and LabelManager.convert_logits_to_segmentation (the call merge_files
    makes) on the result.  A second mean has member 0 stored as float16 (the `avg.dtype != np.float32` branch).  Inputs and
    outputs only."""
    import tempfile
    avg_fn, avg_src = ref_function("ensembling/ensemble.py", "average_probabilities")
    LM, lm_src = ref_function("utilities/label_handling/label_handling.py", "LabelManager",
                              softmax_helper_dim0=lambda x: torch.softmax(x, 0),
                              bounding_box_to_slice=lambda bb: tuple(slice(*i) for i in bb))
    M, K, shape = 3, 3, (6, 7, 9)
    rng = np.random.default_rng(31)
    probs = [torch.softmax(torch.from_numpy((rng.standard_normal((K, *shape)) * 2).astype(np.float32)), 0).numpy()
             for _ in range(M)]
    lm = LM({"background": 0, "a": 1, "b": 2}, None)
    arrs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, first in (("", probs[0]), ("_f16first", probs[0].astype(np.float16))):
            files = []
            for m, p in enumerate([first] + probs[1:]):
                files.append(os.path.join(tmp, f"m{m}{tag}.npz"))
                np.savez(files[-1], probabilities=p)
            mean = avg_fn(files)
            assert mean.dtype == np.float32
            seg = lm.convert_logits_to_segmentation(mean)
            assert np.array_equal(np.asarray(seg), mean.argmax(0)), "the second softmax changed an argmax: pick another seed"
            arrs["mean" + tag] = mean
            arrs["segmentation" + tag] = np.asarray(seg).astype(np.uint8)
    assert len(np.unique(arrs["segmentation"])) == K
    save("ensemble.npz", source=np.array(f"reference {avg_src} on temporary .npz files and {lm_src} "
                                         f"convert_logits_to_segmentation"),
         probabilities=np.stack(probs), first_f16=probs[0].astype(np.float16), **arrs)


if __name__ == "__main__":
    torch.set_num_threads(4)
    if len(sys.argv) > 1 and sys.argv[1] == "ensemble":  # only tests/golden/ensemble.npz
        ensemble_fixture()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "cascade":  # only tests/golden/cascade_transforms.npz
        cascade_fixture()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "topk_loss":  # only tests/golden/topk_loss.npz
        topk_loss_fixture()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "cross_attention":  # only tests/golden/cross_attention.npz
        cross_attention_fixture()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "loader2d":  # only tests/golden/loader2d.json
        loader2d_fixture()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "regions":  # only tests/golden/label_manager.json
        region_label_fixtures()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "extracted":  # only the fixtures compiled out of reference function bodies
        extracted_reference_fixtures()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "oracle-checks":  # only the cases tests/test_oracle.py pins the oracle to
        oracle_check_fixtures()
        sys.exit(0)
    conv_fixtures()
    instnorm_fixtures()
    reference_fixtures()
    extracted_reference_fixtures()
    region_label_fixtures()
    loss_fixtures()
    unet_step_fixture()
    mvd_step_fixture()
    persistence_fixtures()
    oracle_check_fixtures()
    loader2d_fixture()
    cross_attention_fixture()
    topk_loss_fixture()
    cascade_fixture()
    ensemble_fixture()
