"""GPU tests of the fused Adam / AdamW step (csrc/adam.hip, optim.FusedAdam) and of the trainer variants built on it
(nnUNetTrainerAdamMI355, nnUNetTrainerVanillaAdamMI355, nnUNetTrainerCosAnnealMI355).

The oracle is torch.optim.Adam / AdamW on the CPU in fp64 with clip_grad_norm_(12) before step() -- the reference's
optimizers ARE torch's.  Bars are measured (tests/adam_ref.py): per step and tensor kind, max(4 x the error of torch's own fp32
CPU run against fp64, 2^-22 x the tensor's max magnitude).  Measured on one MI355X after 6 steps (AdamW + amsgrad, lr 1e-2;
error / bar): p 1.03e-6 / 4.12e-6, exp_avg 8.3e-9 / 4.8e-8, exp_avg_sq 1.2e-10 / 7.2e-10, max_exp_avg_sq 1.4e-10 / 8.1e-10;
losses of the trainer's steps 2 and 3 against the stepped fp64 oracle: 7.5e-5 / 2.65e-4 and 2.9e-4 / 4.5e-4."""
import copy

import numpy as np
import pytest
import torch

import adam_ref
import bn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def _fused(variant, lr, params, **kw):
    from multimodal_mvd_seg_amd import optim
    v = adam_ref.VARIANTS[variant]
    mine = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in params]
    return mine, optim.FusedAdam(mine, lr, weight_decay=adam_ref.WD, amsgrad=v["amsgrad"],
                                 decoupled_weight_decay=v["decoupled"], max_grad_norm=adam_ref.CLIP, **kw)


def _state(opt, kind):
    """The per-parameter views of one tensor kind, on the host."""
    if kind == "p":
        return [p.detach().cpu() for p in opt.fp.params]
    t = getattr(opt, kind).cpu()
    return [t[o:o + p.numel()].view(p.shape) for p, o in zip(opt.fp.params, opt.fp.offsets)]


def _check(opt, ref, bars, what):
    for kind in adam_ref.KINDS:
        if kind not in ref:
            assert getattr(opt, kind) is None
            continue
        bar, err32, scale = bars[kind]
        got = _state(opt, kind)
        err = max(float((g.double() - r).abs().max()) for g, r in zip(got, ref[kind]))
        print(f"{what} {kind}: max abs err {err:.3e}, bar {bar:.3e} (torch fp32 {err32:.3e}, scale {scale:.3e})")
        assert err <= bar, f"{what} {kind}: max abs err {err:.3e} > bar {bar:.3e} (torch fp32: {err32:.3e}, scale {scale:.3e})"


def _step(opt, mine, grads):
    opt.zero_grad()
    for q, g in zip(mine, grads):
        q.grad.copy_(g.to(DEV))
    opt.step()


# ================================================================================================ kernel
@pytest.mark.parametrize("lr", [1e-2, 3e-4])
@pytest.mark.parametrize("variant", ["adamw_amsgrad", "adam"])
def test_fused_adam_matches_torch_in_fp64_with_clipping(variant, lr):
    c = adam_ref.kernel_case(variant, lr)
    if variant == "adamw_amsgrad":
        # the amsgrad branch is exercised: after the last step the running maximum differs from v in most elements
        last = c["ref"][-1]
        a, b = torch.cat([t.reshape(-1) for t in last["max_exp_avg_sq"]]), torch.cat([t.reshape(-1) for t in last["exp_avg_sq"]])
        assert float((a != b).double().mean()) > 0.5
    clipped = [r["gn"] > adam_ref.CLIP for r in c["ref"]]
    assert clipped == [True, False] * 3                     # both sides of the clip
    mine, opt = _fused(variant, lr, c["params"])
    assert [o % 4 for o in opt.fp.offsets] == [0] * 4 and opt.fp.numel > sum(p.numel() for p in mine)   # alignment padding
    assert opt.fp.numel % 4 == 0 and any(p.numel() % 4 for p in mine)
    for step, (grads, ref, bars) in enumerate(zip(c["grads"], c["ref"], c["bars"])):
        _step(opt, mine, grads)
        gn = float(opt.grad_norm())
        assert abs(gn - ref["gn"]) <= 1e-4 * ref["gn"], (step, gn, ref["gn"])
        _check(opt, ref, bars, f"{variant} lr {lr:g} step {step + 1}")
        assert int(opt.step_dev) == opt._steps == step + 1


def test_scalar_tail_without_padding():
    """FlatParams pads every tensor to four floats, so FusedAdam.step() always passes n % 4 == 0 and the kernel's scalar tail
    never runs through it.  Here the entry point itself is given n = 1023 on a 1024-element buffer: the tail takes the last
    three elements and leaves the one behind them alone."""
    import ctypes
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, query
    n = 1023
    params, grads = adam_ref.kernel_inputs(shapes=[(n,)], steps=2, seed=11)
    r64, _ = adam_ref.run_torch("adamw_amsgrad", 1e-2, params, grads, torch.float64)
    r32, _ = adam_ref.run_torch("adamw_amsgrad", 1e-2, params, grads, torch.float32)
    mine, opt = _fused("adamw_amsgrad", 1e-2, params)
    assert opt.fp.numel == 1024
    guard = [float(t[n]) for t in (opt.fp.flat, opt.exp_avg, opt.exp_avg_sq, opt.max_exp_avg_sq)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = ops._Workspace.get(query("mvd_sumsq_workspace_bytes", n), DEV)
    opt.sync_hyper()
    for step in range(2):
        opt.fp.grad[:n].copy_(grads[step][0].to(DEV))
        call("mvd_grad_sumsq", P(opt.fp.grad), P(opt.sumsq), n, P(ws), ws.numel(), s)
        call("mvd_adam_step", P(opt.fp.flat), P(opt.fp.grad), P(opt.exp_avg), P(opt.exp_avg_sq), P(opt.max_exp_avg_sq),
             P(opt.sumsq), n, P(opt.hyper), P(opt.step_dev), 1, s)
        bars = {k: adam_ref.bar(r64[step][k], r32[step][k]) for k in adam_ref.KINDS}
        _check(opt, r64[step], bars, f"n = {n}, step {step + 1}")
    assert int(opt.step_dev) == 2
    # the element behind the tail was not touched
    assert guard == [float(t[n]) for t in (opt.fp.flat, opt.exp_avg, opt.exp_avg_sq, opt.max_exp_avg_sq)]


def test_entry_point_refuses_bad_arguments():
    import ctypes
    from multimodal_mvd_seg_amd._lib import load
    lib = load()
    x = torch.zeros(16, device=DEV)
    h = torch.zeros(16, dtype=torch.float64, device=DEV)
    c = torch.zeros(1, dtype=torch.int64, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731
    assert lib.mvd_adam_step(P(x), P(x), P(x), P(x), None, P(x), 0, P(h), P(c), 1, None) == 2
    assert b"bad arguments" in lib.mvd_last_error()
    assert lib.mvd_adam_step(P(x), P(x), None, P(x), None, P(x), 16, P(h), P(c), 1, None) == 2
    assert lib.mvd_adam_step(P(x), P(x), P(x), P(x), None, P(x), 16, None, P(c), 1, None) == 2
    assert lib.mvd_adam_step(P(x), P(x), P(x), P(x), None, P(x), 16, P(h), None, 1, None) == 2
    assert lib.mvd_adam_step(P(x), P(x), P(x), P(x), P(x, 4), P(x), 8, P(h), P(c), 1, None) == 2
    assert b"16-byte aligned" in lib.mvd_last_error()
    assert lib.mvd_adam_step(P(x, 4), P(x), P(x), P(x), None, P(x), 8, P(h), P(c), 1, None) == 2
    torch.cuda.synchronize()
    assert int(c) == 0 and not x.any()


def test_grid_stride_loop_past_one_sweep_of_the_capped_grid():
    c = adam_ref.big_case()
    assert adam_ref.BIG_N == 4096 * 256 * 4 + 1027
    mine, opt = _fused("adamw_amsgrad", 1e-2, c["params"])
    assert opt.fp.numel // 4 > 4096 * 256       # at least one thread takes a second trip
    for step, (grads, ref, bars) in enumerate(zip(c["grads"], c["ref"], c["bars"])):
        _step(opt, mine, grads)
        _check(opt, ref, bars, f"big step {step + 1}")


@pytest.mark.parametrize("variant", ["adamw_amsgrad", "adam"])
def test_fused_adam_grad_scale_is_the_data_parallel_mean(variant):
    """The twin of test_fused_sgd_grad_scale_is_the_data_parallel_mean, at its tolerances."""
    torch.manual_seed(1)
    base = [torch.randn(s) for s in [(40, 9, 3), (7,), (515,)]]
    for gmag in (40.0, 0.02):
        a, oa = _fused(variant, 1e-2, base)
        b, ob = _fused(variant, 1e-2, base)
        oa.grad_scale = 0.25
        for step in range(3):
            oa.zero_grad()
            ob.zero_grad()
            for p, q in zip(a, b):
                g = (torch.randn(p.shape) * gmag).to(DEV)
                p.grad.copy_(g)            # the SUM over 4 ranks
                q.grad.copy_(g * 0.25)     # the mean, taken by a separate pass
            oa.step()
            ob.step()
            assert abs(float(oa.grad_norm()) - float(ob.grad_norm())) <= 1e-6 * float(ob.grad_norm())
            assert (float(ob.grad_norm()) > 12) == (gmag == 40.0)
            for p, q in zip(a, b):
                err = (p.detach() - q.detach()).abs().cpu()
                assert bool((err <= 1e-7 + 1e-6 * q.detach().abs().cpu()).all()), f"param step {step}: {float(err.max()):.3e}"


def test_checkpoint_exchange_with_torch_adamw():
    """Ours -> torch.optim.AdamW and torch -> a fresh FusedAdam after 2 device steps: both then take the same third step."""
    from multimodal_mvd_seg_amd import optim
    params, grads = adam_ref.kernel_inputs(steps=3, seed=5)
    r64, _ = adam_ref.run_torch("adamw_amsgrad", 1e-2, params, grads, torch.float64)
    r32, _ = adam_ref.run_torch("adamw_amsgrad", 1e-2, params, grads, torch.float32)
    bars = {k: adam_ref.bar(r64[2][k], r32[2][k]) for k in adam_ref.KINDS}
    named = [(f"w{i}", p) for i, p in enumerate(params)]
    mine = [(n, torch.nn.Parameter(p.clone().to(DEV))) for n, p in named]
    opt = optim.FusedAdam(optim.FlatParams(mine[::-1]), 1e-2, weight_decay=adam_ref.WD, amsgrad=True,
                          decoupled_weight_decay=True, max_grad_norm=adam_ref.CLIP)
    by_name = dict(mine)
    for step in range(2):
        _step(opt, [by_name[n] for n, _ in named], grads[step])
    tsd = opt.to_torch_state_dict(mine)
    # torch's side: fp64 parameters as the device left them, the exchanged state, the third step
    tp = [torch.nn.Parameter(q.detach().cpu().double()) for _, q in mine]
    topt = torch.optim.AdamW(tp, lr=1.0, amsgrad=True)
    topt.load_state_dict(copy.deepcopy(tsd))       # (torch keeps the 'step' tensors it is given and advances them in place)
    assert topt.param_groups[0]["lr"] == 1e-2 and topt.param_groups[0]["weight_decay"] == adam_ref.WD
    assert all(float(topt.state[p]["step"]) == 2.0 and topt.state[p]["exp_avg"].dtype == torch.float64 for p in tp)
    for p, g in zip(tp, grads[2]):
        p.grad = g.double()
    torch.nn.utils.clip_grad_norm_(tp, adam_ref.CLIP)
    topt.step()
    # our side: a FRESH optimizer (another layout order) loaded from torch's format
    fresh = [(n, torch.nn.Parameter(q.detach().clone())) for n, q in mine]
    fopt = optim.FusedAdam(optim.FlatParams(fresh), 1.0, amsgrad=True, decoupled_weight_decay=True,
                           max_grad_norm=adam_ref.CLIP)
    fopt.load_torch_state_dict(tsd, fresh)
    assert fopt._steps == 2 and int(fopt.step_dev) == 2 and fopt.param_groups[0]["weight_decay"] == adam_ref.WD
    _step(fopt, [q for _, q in fresh], grads[2])
    assert int(fopt.step_dev) == 3
    for (n, q), p in zip(fresh, tp):
        err = float((q.detach().cpu().double() - p.detach()).abs().max())
        print(f"{n}: {err:.3e} (bar {bars['p'][0]:.3e})")
        assert err <= bars["p"][0], (n, err, bars["p"])
    # and the state the continued device optimizer holds is the one-process run's
    _step(opt, [by_name[n] for n, _ in named], grads[2])
    for (n, q), (_, f) in zip(mine, fresh):
        assert torch.equal(q.detach(), f.detach()), n


# ================================================================================================ trainers
def _trainer(cls_name, precision="fp32", graph=None, num_epochs=None):
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(bn_ref.PATCH, bn_ref.STRIDES, batch_size=bn_ref.BATCH)
    tr = getattr(trainer, cls_name)(plans, "3d_fullres", 0, bn_ref.DATASET_JSON, device=DEV)
    tr.precision = precision
    if graph is not None:
        tr.use_hip_graph = graph
    if num_epochs is not None:
        tr.num_epochs = num_epochs
    tr.initialize()
    tr.network.load_state_dict(adam_ref.oracle_net().state_dict(), strict=True)
    tr.optimizer.fp.invalidate_packs()
    return tr


def _gbatch(seed=bn_ref.BATCH_SEED):
    b = bn_ref.batch(seed)
    return {"data": b["data"].to(DEV), "target": [t.to(DEV) for t in b["target"]]}


@pytest.mark.parametrize("cls_name,precision", [("nnUNetTrainerAdamMI355", "fp32"), ("nnUNetTrainerAdamMI355", "bf16"),
                                                ("nnUNetTrainerVanillaAdamMI355", "fp32")])
def test_graphed_adam_step_follows_schedule_and_counter_bit_for_bit(cls_name, precision):
    a = _trainer(cls_name, precision, graph=False)
    b = _trainer(cls_name, precision, graph=True)
    assert b.hip_graph_warmup == 3 and type(a.optimizer).__name__ == "FusedAdam"
    batches = [_gbatch(100 + i) for i in range(8)]
    for tr in (a, b):
        tr.on_train_epoch_start()
    for i, bt in enumerate(batches):
        la = np.asarray(a.train_step(bt)["loss"]).copy()
        lb = np.asarray(b.train_step(bt)["loss"]).copy()
        assert np.array_equal(la, lb), f"loss of step {i}: eager {la} graph {lb}"
        if i == 3:      # after step 4 (3 eager + the capture): the schedule moves, validation, a state reload; 4 replays follow
            assert b._step_graph is not None and b._step_graph["graph"] is not None, "the step was never captured"
            for tr in (a, b):
                lr0 = tr.optimizer.param_groups[0]["lr"]
                tr.lr_scheduler.step(1)
                assert tr.optimizer.param_groups[0]["lr"] < lr0
                tr.validation_step(batches[0])
                tr.network.load_state_dict({k: v.clone() for k, v in tr.network.state_dict().items()}, strict=True)
    torch.cuda.synchronize()
    assert a._step_graph is None
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    for (k, x), (_, y) in zip(a.optimizer._buffers(), b.optimizer._buffers()):
        assert torch.equal(x, y), k
        assert bool(x.any())
    assert (a.optimizer.max_exp_avg_sq is not None) == (cls_name == "nnUNetTrainerAdamMI355")
    for tr in (a, b):
        assert int(tr.optimizer.step_dev) == tr.optimizer._steps == 8
        assert tr.optimizer.state_dict()["steps"] == 8


def test_trainer_wiring_against_the_oracle_optimizer_on_device_gradients():
    """Layout, name mapping, clip and update of nnUNetTrainerAdamMI355: the device gradients of each step, in fp64 and in
    network.parameters() order, drive torch.optim.AdamW(amsgrad=True) + clip_grad_norm_(12) on an fp64 copy of the initial
    parameters (and an fp32 copy, for the bars).  (Parameters after a step cannot be held to a NETWORK-level fp64 oracle:
    Adam's first updates are ~ lr * sign(g), so a gradient below the fp32 backward's error moves its parameter by up to lr
    differently in any fp32 evaluation.)"""
    tr = _trainer("nnUNetTrainerAdamMI355", graph=False)
    tr.on_train_epoch_start()
    named = list(tr.network.named_parameters())
    assert [n for n, _s, _o in tr.optimizer.fp.layout()] != [n for n, _ in named], "execution order == definition order here"
    p64 = [torch.nn.Parameter(p.detach().cpu().double()) for _, p in named]
    p32 = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in named]
    o64 = torch.optim.AdamW(p64, lr=1e-2, weight_decay=3e-5, amsgrad=True)
    o32 = torch.optim.AdamW(p32, lr=1e-2, weight_decay=3e-5, amsgrad=True)
    gb = _gbatch()
    for step in range(3):
        tr.optimizer.zero_grad()
        l = tr.loss(tr.network(gb["data"]), gb["target"])
        l.backward()
        grads = [p.grad.detach().cpu().clone() for _, p in named]
        for ps, opt, dt in ((p64, o64, torch.float64), (p32, o32, torch.float32)):
            for p, g in zip(ps, grads):
                p.grad = g.to(dt)
            gn = torch.nn.utils.clip_grad_norm_(ps, 12)
            opt.step()
        tr.optimizer.step()
        assert abs(float(tr.optimizer.grad_norm()) - float(gn)) <= 1e-4 * float(gn)
        ref = [p.detach() for p in p64]
        bar, err32, scale = adam_ref.bar(ref, [p.detach() for p in p32])
        worst = 0.0
        for (n, p), r in zip(named, ref):
            err = float((p.detach().cpu().double() - r).abs().max())
            worst = max(worst, err)
            assert err <= bar, f"step {step + 1}, {n}: max abs err {err:.3e} > bar {bar:.3e} (torch fp32: {err32:.3e})"
        print(f"step {step + 1}: worst parameter err {worst:.3e}, bar {bar:.3e} (torch fp32 {err32:.3e}, scale {scale:.3e})")
    assert int(tr.optimizer.step_dev) == 3


def test_adam_trainer_loss_trajectory_against_the_stepped_fp64_oracle():
    r = adam_ref.loss_trajectory()
    tr = _trainer("nnUNetTrainerAdamMI355")
    tr.on_train_epoch_start()
    gb = _gbatch()
    for step, (ref, bar, l32) in enumerate(zip(r["losses"], r["bars"], r["fp32"])):
        l = float(tr.train_step(gb)["loss"])
        print(f"loss of step {step + 1}: {l:.7f}, fp64 oracle {ref:.7f} (err {abs(l - ref):.3e}, bar {bar:.3e}; torch fp32 "
              f"{abs(l32 - ref):.3e})")
        assert abs(l - ref) <= bar, (step + 1, l, ref, bar)
    assert r["losses"][2] < r["losses"][0]        # it trains


def test_cos_anneal_trainer_is_the_sgd_trainer_with_the_cosine_learning_rate():
    import math
    a = _trainer("nnUNetTrainerCosAnnealMI355", num_epochs=4)
    b = _trainer("nnUNetTrainerMI355", num_epochs=4)
    assert type(a.optimizer) is type(b.optimizer) and a.lr_scheduler.T_max == 4
    batches = [_gbatch(200 + i) for i in range(4)]
    for epoch in (0, 1):
        want = 1e-2 * (1 + math.cos(math.pi * epoch / 4)) / 2
        a.current_epoch = b.current_epoch = epoch
        a.on_train_epoch_start()
        b.on_train_epoch_start()
        assert a.optimizer.param_groups[0]["lr"] == want
        b.optimizer.param_groups[0]["lr"] = want          # by hand, over PolyLR's value
        for bt in batches[2 * epoch:2 * epoch + 2]:
            la, lb = a.train_step(bt)["loss"], b.train_step(bt)["loss"]
            assert np.array_equal(la, lb)
    assert want < 1e-2
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    assert torch.equal(a.optimizer.momentum_buffer, b.optimizer.momentum_buffer)
