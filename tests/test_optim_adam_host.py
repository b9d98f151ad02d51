"""CPU tests of the Adam / AdamW / cosine-annealing host side (optim.FusedAdam, optim.CosineAnnealingLR and the trainer
variants of variants/optimizer/nnUNetTrainerAdam.py and variants/lr_schedule/nnUNetTrainerCosAnneal.py).  No kernel runs here;
tests/test_gpu_adam.py holds the arithmetic to torch.optim in fp64."""
import math
import warnings

import pytest
import torch
from torch import nn

from multimodal_mvd_seg_amd import optim, trainer

DATASET_JSON = {"channel_names": {"0": "m0"}, "labels": {"background": 0, "a": 1}}


def _toy():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(3, 5), nn.Linear(5, 5), nn.Linear(5, 2), nn.Linear(2, 7, bias=False))


def _configured(cls):
    plans = trainer.make_plans((16, 16, 16), [[1, 1, 1], [2, 2, 2]])
    tr = cls(plans, "3d_fullres", 0, DATASET_JSON, device=torch.device("cuda"))   # (a device OBJECT: nothing touches a GPU)
    tr.network = _toy()
    return tr, tr.configure_optimizers()


TORCH_KEYS = ("lr", "betas", "eps", "weight_decay", "amsgrad")
ADAM_TRAINERS = [("nnUNetTrainerAdamMI355", 1e-2, True), ("nnUNetTrainerAdam1en3MI355", 1e-3, True),
                 ("nnUNetTrainerAdam3en4MI355", 3e-4, True), ("nnUNetTrainerVanillaAdamMI355", 1e-2, False),
                 ("nnUNetTrainerVanillaAdam1en3MI355", 1e-3, False), ("nnUNetTrainerVanillaAdam3en4MI355", 3e-4, False)]


@pytest.mark.parametrize("name,lr,adamw", ADAM_TRAINERS)
def test_adam_trainers_configure_the_reference_classes_arguments(name, lr, adamw):
    """nnUNetTrainerAdam.py: AdamW(lr=initial_lr, weight_decay=3e-5, amsgrad=True) / Adam(lr=initial_lr, weight_decay=3e-5),
    everything else torch's default -- read off a torch optimizer built with exactly those arguments."""
    import multimodal_mvd_seg_amd as pkg
    cls = getattr(pkg, name)                     # exported beside nnUNetTrainerBNMI355
    assert cls is getattr(trainer, name) and name in pkg.__all__
    tr, (opt, sched) = _configured(cls)
    w = nn.Parameter(torch.zeros(1))
    ref = (torch.optim.AdamW([w], lr=lr, weight_decay=3e-5, amsgrad=True) if adamw
           else torch.optim.Adam([w], lr=lr, weight_decay=3e-5)).param_groups[0]
    assert isinstance(opt, optim.FusedAdam) and isinstance(sched, optim.PolyLRScheduler)
    g = opt.param_groups[0]
    for k in TORCH_KEYS:
        assert g[k] == ref[k], (k, g[k], ref[k])
    assert g["decoupled_weight_decay"] is adamw and g["amsgrad"] is adamw
    assert (opt.max_exp_avg_sq is not None) == adamw
    assert opt.max_grad_norm == 12 and opt.grad_scale == 1.0
    assert sched.max_steps == tr.num_epochs == 200 and sched.initial_lr == lr
    assert g["params"] == opt.fp.params and len(opt.fp.params) == 7
    assert [n for n, _s, _o in opt.fp.layout()] == [n for n, _ in tr.network.named_parameters()]
    # the schedule drives the same key the kernel's scalars are read from
    sched.step(100)
    assert g["lr"] == lr * (1 - 100 / 200) ** 0.9 and opt._hyper_values()[0] == g["lr"]


def test_base_and_cosine_trainers_configure_sgd():
    _, (opt, sched) = _configured(trainer.nnUNetTrainerMI355)
    assert type(opt) is optim.FusedSGDNesterov and type(sched) is optim.PolyLRScheduler
    assert opt.param_groups[0] == {'lr': 1e-2, 'weight_decay': 3e-5, 'momentum': 0.99, 'nesterov': True,
                                   'params': opt.fp.params} and opt.max_grad_norm == 12
    tr, (opt, sched) = _configured(trainer.nnUNetTrainerCosAnnealMI355)
    assert type(opt) is optim.FusedSGDNesterov and type(sched) is optim.CosineAnnealingLR
    assert {k: v for k, v in opt.param_groups[0].items() if k != 'params'} == \
        {'lr': 1e-2, 'weight_decay': 3e-5, 'momentum': 0.99, 'nesterov': True}
    assert sched.T_max == tr.num_epochs and sched.eta_min == 0.0


def test_fused_adam_constructs_on_cpu_parameters_and_refuses_to_step_there():
    net = _toy()
    opt = optim.FusedAdam(net.parameters(), 1e-3)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (1e-3, (0.9, 0.999), 1e-8, 0, False)
    assert opt.max_grad_norm == 12.0 and opt.max_exp_avg_sq is None and opt._steps == 0 and int(opt.step_dev) == 0
    assert opt.exp_avg.shape == opt.exp_avg_sq.shape == opt.fp.flat.shape
    for surface in ("fp", "param_groups", "max_grad_norm", "grad_scale", "sumsq", "zero_grad", "grad_norm", "step",
                    "use_device_hyper", "sync_hyper", "note_replayed_step", "state_dict", "load_state_dict"):
        assert hasattr(opt, surface), surface
    opt.zero_grad()
    with pytest.raises(RuntimeError, match="MI355X only"):
        opt.step()
    assert opt._steps == 0
    with pytest.raises(ValueError, match="beta"):
        optim.FusedAdam(net.parameters(), 1e-3, betas=(1.0, 0.999))


def _stepped_torch(named, amsgrad=True, steps=2):
    ref = torch.optim.AdamW([p for _, p in named], lr=1e-2, weight_decay=3e-5, amsgrad=amsgrad)
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        for _, p in named:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    return ref


def test_torch_state_round_trip_through_a_reversed_flat_layout():
    """torch -> ours -> torch: every tensor and every `step` comes back equal; the flat buffers are in REVERSED order, so the
    state of parameter i has to travel by name."""
    net = _toy()
    named = list(net.named_parameters())[:4]
    sd = _stepped_torch(named).state_dict()
    opt = optim.FusedAdam(optim.FlatParams(named[::-1]), lr=1.0, weight_decay=3e-5, amsgrad=True, decoupled_weight_decay=True)
    opt.load_torch_state_dict(sd, named)
    assert opt._steps == 2 and int(opt.step_dev) == 2 and opt.param_groups[0]["lr"] == 1e-2
    # it landed on the right parameter
    for i, (n, p) in enumerate(named):
        o = opt.fp.offsets[opt.fp.names.index(n)]
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert torch.equal(getattr(opt, k)[o:o + p.numel()].view(p.shape), sd["state"][i][k]), (n, k)
    back = opt.to_torch_state_dict(named)
    assert set(back["state"]) == set(sd["state"]) == {0, 1, 2, 3}
    for i, st in sd["state"].items():
        assert set(back["state"][i]) == set(st) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
        for k, v in st.items():
            assert back["state"][i][k].dtype == v.dtype and torch.equal(back["state"][i][k], v), (i, k)
    assert back["param_groups"][0]["params"] == sd["param_groups"][0]["params"]
    for k in TORCH_KEYS + ("decoupled_weight_decay",):
        assert back["param_groups"][0][k] == sd["param_groups"][0][k], k
    # and torch takes it
    fresh = torch.optim.AdamW([p for _, p in named], lr=1.0, amsgrad=True)
    fresh.load_state_dict(back)
    assert fresh.param_groups[0]["lr"] == 1e-2 and float(fresh.state[named[2][1]]["step"]) == 2.0
    # a fresh optimizer maps to torch's empty state, and back
    new = optim.FusedAdam(optim.FlatParams(named), lr=1e-2, amsgrad=True)
    assert new.to_torch_state_dict(named)["state"] == {}
    opt.load_torch_state_dict(new.to_torch_state_dict(named), named)
    assert opt._steps == 0 and int(opt.step_dev) == 0 and not opt.exp_avg.any() and not opt.max_exp_avg_sq.any()


def test_torch_state_that_cannot_be_one_fused_state_is_refused():
    net = _toy()
    named = list(net.named_parameters())[:4]
    sd = _stepped_torch(named).state_dict()
    opt = optim.FusedAdam(optim.FlatParams(named), lr=1e-2, amsgrad=True)
    opt.exp_avg.fill_(7.0)
    bad = {"state": {i: dict(st) for i, st in sd["state"].items()}, "param_groups": sd["param_groups"]}
    bad["state"][2]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="step counts differ"):
        opt.load_torch_state_dict(bad, named)
    assert opt._steps == 0 and int(opt.step_dev) == 0 and bool((opt.exp_avg == 7.0).all())      # nothing half-loaded
    no_ams = _stepped_torch(named, amsgrad=False).state_dict()
    with pytest.raises(ValueError, match="max_exp_avg_sq"):
        opt.load_torch_state_dict(no_ams, named)
    with pytest.raises(ValueError, match="one to one"):
        opt.load_torch_state_dict(sd, named[:3])
    assert bool((opt.exp_avg == 7.0).all())


def _fill(opt):
    """slice of parameter i of every state buffer <- (i + 1) * (1, 10, 100); returns {id(parameter): i + 1}"""
    want = {}
    for i, (p, o) in enumerate(zip(opt.fp.params, opt.fp.offsets)):
        for (_k, t), f in zip(opt._buffers(), (1.0, 10.0, 100.0)):
            t[o:o + p.numel()] = (i + 1) * f
        want[id(p)] = float(i + 1)
    return want


def test_own_state_format_carries_its_layout_like_the_sgd_momentum():
    """What test_optimizer_state_carries_its_parameter_layout_and_is_never_misassigned_silently demands of the momentum, for
    every Adam buffer."""
    net = nn.Sequential(nn.Linear(3, 5), nn.Linear(5, 5), nn.Linear(5, 2))   # two (5,) biases
    named = list(net.named_parameters())
    a = optim.FusedAdam(optim.FlatParams(named), 1e-2, amsgrad=True)
    want = _fill(a)
    a._set_steps(3)
    sd = a.state_dict()
    assert set(sd) == {"exp_avg", "exp_avg_sq", "max_exp_avg_sq", "steps", "layout", "param_groups"}
    assert sd["steps"] == 3 and [n for n, _s, _o in sd["layout"]] == [n for n, _ in named]
    assert "params" not in sd["param_groups"][0] and sd["param_groups"][0]["amsgrad"] is True
    b = optim.FusedAdam(optim.FlatParams(named[::-1]), 1e-3, amsgrad=True)
    assert sd["exp_avg"].numel() == b.exp_avg.numel()
    b.load_state_dict(sd)
    assert b._steps == 3 and int(b.step_dev) == 3 and b.param_groups[0]["lr"] == 1e-2
    for p, o in zip(b.fp.params, b.fp.offsets):
        for (k, t), f in zip(b._buffers(), (1.0, 10.0, 100.0)):
            got = t[o:o + p.numel()]
            assert torch.equal(got, torch.full_like(got, want[id(p)] * f)), f"{k} landed on another parameter"
    a2 = optim.FusedAdam(optim.FlatParams(named), 1e-2, amsgrad=True)
    a2.load_state_dict(sd)
    for k, t in a2._buffers():
        assert torch.equal(t, sd[k]), k
    # without names: loud, nothing half-loaded
    plain = [p for _, p in named]
    c = optim.FusedAdam(optim.FlatParams(plain), 1e-2, amsgrad=True)
    _fill(c)
    d = optim.FusedAdam(optim.FlatParams(plain[::-1]), 1e-2, amsgrad=True)
    with pytest.raises(ValueError, match="layout mismatch"):
        d.load_state_dict(c.state_dict())
    assert not d.exp_avg.any() and not d.exp_avg_sq.any() and d._steps == 0 and int(d.step_dev) == 0
    e = optim.FusedAdam(optim.FlatParams([("x." + n, p) for n, p in named[::-1]]), 1e-2, amsgrad=True)
    with pytest.raises(ValueError, match="layout mismatch"):
        e.load_state_dict(sd)
    with pytest.raises(ValueError, match="layout mismatch"):
        b.load_state_dict(dict(sd, exp_avg_sq=sd["exp_avg_sq"][:-4]))
    # a state saved without amsgrad has no max_exp_avg_sq to give
    f = optim.FusedAdam(optim.FlatParams(named), 1e-2)
    assert set(f.state_dict()) == {"exp_avg", "exp_avg_sq", "steps", "layout", "param_groups"}
    with pytest.raises(ValueError, match="max_exp_avg_sq"):
        a2.load_state_dict(f.state_dict())


def test_cosine_annealing_is_torchs_closed_form():
    w = nn.Parameter(torch.zeros(1))
    topt = torch.optim.SGD([w], lr=1e-2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tsch = torch.optim.lr_scheduler.CosineAnnealingLR(topt, T_max=10)
        mine_opt = optim.FusedSGDNesterov([nn.Parameter(torch.zeros(1))], 1e-2)
        sch = optim.CosineAnnealingLR(mine_opt, T_max=10)
        assert mine_opt.param_groups[0]["lr"] == 1e-2
        for e in (0, 1, 5, 10, 3):
            tsch.step(e)
            sch.step(e)
            want, got = topt.param_groups[0]["lr"], mine_opt.param_groups[0]["lr"]
            assert abs(got - want) <= 1e-15 * abs(want), (e, got, want)
            assert abs(got - 1e-2 * (1 + math.cos(math.pi * e / 10)) / 2) <= 1e-17
    # without an argument it counts by itself, as PolyLRScheduler does
    sch2 = optim.CosineAnnealingLR(mine_opt, T_max=10)
    sch2.step()
    assert abs(mine_opt.param_groups[0]["lr"] - sch2.base_lrs[0] * (1 + math.cos(math.pi * 1 / 10)) / 2) <= 1e-17
