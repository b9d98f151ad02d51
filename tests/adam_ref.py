"""TEST INFRASTRUCTURE: the shared references of the Adam / AdamW tests.

The reference's optimizers ARE torch.optim.Adam / AdamW (variants/optimizer/nnUNetTrainerAdam.py), preceded by
clip_grad_norm_(parameters, 12) in train_step, so torch on the CPU in fp64 is the oracle.

Tolerance rule (measured, not chosen): the same recipe is also run by torch on the CPU in fp32.  A tensor kind (parameters,
exp_avg, exp_avg_sq, max_exp_avg_sq; all parameters of the case together, as they are ONE flat buffer on the device) is held,
after every step, to  max(4 x the fp32 run's max error against fp64, 2^-22 x the fp64 tensor's max magnitude):  4 for a
different but equally valid fp32 evaluation order, the floor (one fp32 ulp of the largest entry, twice over) for tensors torch
happens to hit exactly."""
import functools

import torch

SHAPES = [(33, 7, 3), (5,), (1023,), (64, 64)]      # odd sizes, alignment padding, a scalar tail
VARIANTS = {"adamw_amsgrad": dict(cls=torch.optim.AdamW, amsgrad=True, decoupled=True),
            "adam": dict(cls=torch.optim.Adam, amsgrad=False, decoupled=False)}
WD, CLIP, STEPS = 3e-5, 12, 6
KINDS = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
FLOOR = 2.0 ** -22


def bar(ref64, run32):
    """The bar of one tensor kind: lists of fp64 and fp32 tensors (one per parameter)."""
    err = max(float((b.double() - a).abs().max()) for a, b in zip(ref64, run32))
    scale = max(float(a.abs().max()) for a in ref64)
    return max(4.0 * err, FLOOR * scale), err, scale


def run_torch(variant, lr, params, grads, dtype):
    """torch.optim on the CPU in `dtype`: clip_grad_norm_(CLIP) + step() per entry of `grads` (a list over steps of lists
    over parameters).  Returns per step {'p', 'exp_avg', 'exp_avg_sq'[, 'max_exp_avg_sq']: lists of tensors, 'gn': norm}."""
    v = VARIANTS[variant]
    ps = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in params]
    opt = v["cls"](ps, lr=lr, weight_decay=WD, amsgrad=v["amsgrad"])
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.detach().to(dtype).clone()
        gn = torch.nn.utils.clip_grad_norm_(ps, CLIP)
        opt.step()
        rec = {"p": [p.detach().clone() for p in ps], "gn": float(gn)}
        for k in KINDS[1:]:
            if k in opt.state[ps[0]]:
                rec[k] = [opt.state[p][k].clone() for p in ps]
        out.append(rec)
    return out, opt


def kernel_inputs(shapes=SHAPES, steps=STEPS, seed=0):
    """Initial parameters and per-step gradients: randn x 30 on even steps (clipped), randn x 0.01 on odd ones (not)."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * (30.0 if step % 2 == 0 else 0.01) for s in shapes] for step in range(steps)]
    return params, grads


@functools.lru_cache(maxsize=None)
def kernel_case(variant, lr):
    """Computed once per session, shared and left unchanged: inputs, the fp64 oracle per step, and the bars per step and kind."""
    params, grads = kernel_inputs()
    r64, _ = run_torch(variant, lr, params, grads, torch.float64)
    r32, _ = run_torch(variant, lr, params, grads, torch.float32)
    bars = [{k: bar(a[k], b[k]) for k in KINDS if k in a} for a, b in zip(r64, r32)]
    return {"params": params, "grads": grads, "ref": r64, "bars": bars}


BIG_N = 4096 * 256 * 4 + 1027      # one element more than one sweep of the capped grid (4096 blocks x 256 threads x 4), + a tail


@functools.lru_cache(maxsize=None)
def big_case():
    g = torch.Generator().manual_seed(3)
    params = [torch.randn(BIG_N, generator=g)]
    grads = [[torch.randn(BIG_N, generator=g) * (30.0 if step % 2 == 0 else 0.01)] for step in range(2)]
    r64, _ = run_torch("adamw_amsgrad", 1e-2, params, grads, torch.float64)
    r32, _ = run_torch("adamw_amsgrad", 1e-2, params, grads, torch.float32)
    bars = [{k: bar(a[k], b[k]) for k in KINDS if k in a} for a, b in zip(r64, r32)]
    return {"params": params, "grads": grads, "ref": r64, "bars": bars}


# ---------------------------------------------------------------------------------------------- the tiny network
def oracle_net(dtype=torch.float32):
    """The BatchNorm tests' network with its InstanceNorm left in place: 3 stages, 32/64/128, 4 channels (bn_ref constants)."""
    import bn_ref
    from oracle import unet_oracle as UO
    return UO.build_plainconv_unet(bn_ref.IN_CH, bn_ref.CLASSES, 3, bn_ref.STRIDES, features_per_stage=bn_ref.FEATURES,
                                   deep_supervision=True, seed=bn_ref.NET_SEED).to(dtype)


def _loss_run(dtype, steps):
    import bn_ref
    from oracle import loss_oracle as LO, step_oracle as SO
    net = oracle_net(dtype)
    b = bn_ref.batch()
    b = {"data": b["data"].to(dtype), "target": [t.to(dtype) for t in b["target"]]}
    loss_fn = LO.build_loss(len(b["target"]))
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2, weight_decay=WD, amsgrad=True)
    return [float(SO.train_step(net, loss_fn, opt, b)[0]) for _ in range(steps)]


@functools.lru_cache(maxsize=None)
def loss_trajectory(steps=3):
    """Losses of `steps` oracle train steps (oracle.step_oracle.train_step with AdamW(amsgrad)) in fp64, and the bar of every
    step: 1e-5 x max(1, |loss|) before any update (the network tests' bar); afterwards max(4 x the deviation of torch's own
    fp32 CPU run of the same recipe, 1e-5)."""
    l64, l32 = _loss_run(torch.float64, steps), _loss_run(torch.float32, steps)
    bars = [1e-5 * max(1.0, abs(l64[0]))] + [max(4.0 * abs(a - b), 1e-5) for a, b in zip(l64[1:], l32[1:])]
    return {"losses": l64, "fp32": l32, "bars": bars}
