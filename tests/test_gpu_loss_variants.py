"""GPU tests of the six loss trainer variants on a tiny 3-D and a tiny 2-D plan: the first step's loss is the
loss module applied to the network's outputs and matches the fp64 restatement of the trainer's composition
(tests/topk_ref.py) at the loss bar; the graphed step equals the eager step bit for bit, with validation_step calls in
between; nnUNetTrainerCELossMI355 with an ignore label and nnUNetTrainerDiceLossMI355 with regions follow the oracle
network under their fp64 restatements.  Bars: DESIGN 8 / 20 (loss 1e-5 relative, parameters after steps 1e-5)."""
import numpy as np
import pytest
import torch

import topk_ref as TR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CH = {"channel_names": {"0": "a", "1": "b"}}
PLAIN = dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3})
IGNORE = dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3, "ignore": 4})
REGIONS_JSON = dict(CH, labels={"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, regions_class_order=[1, 2, 3])
REGIONS = [(1, 2, 3), (2, 3), 3]
PLANS = {
    "3d": dict(patch=(32, 32, 32), strides=[[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2]], configuration="3d_fullres"),
    "2d": dict(patch=(32, 32), strides=[[1, 1], [2, 2], [2, 2]], configuration="2d"),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def make_trainer(name, dim="3d", dataset=PLAIN, graph=False, batch_dice=False, precision="fp32", base=8):
    from multimodal_mvd_seg_amd import trainer
    p = PLANS[dim]
    plans = trainer.make_plans(p["patch"], p["strides"], batch_size=2, base_features=base, max_features=4 * base, batch_dice=batch_dice,
                               configuration=p["configuration"])
    tr = getattr(trainer, name)(plans, p["configuration"], 0, dataset, device=DEV)
    tr.use_hip_graph = graph
    tr.hip_graph_warmup = 1
    tr.precision = precision
    torch.manual_seed(0)
    tr.initialize()
    return tr


def batch(dim, seed, nlab=4):
    """data + float label-map targets per deep-supervision level, the top one downsampled by picking voxels"""
    g = torch.Generator().manual_seed(seed)
    patch = PLANS[dim]["patch"]
    nd = len(patch)
    data = torch.rand((2, 2, *patch), generator=g)
    top = torch.randint(0, nlab, (2, 1, *[8] * nd), generator=g).float()
    for ax in range(nd):
        top = top.repeat_interleave(4, 2 + ax)
    levels = len(PLANS[dim]["strides"]) - 1
    sl = lambda s: (slice(None), slice(None)) + (slice(None, None, s),) * nd
    return {'data': data, 'target': [top[sl(2 ** i)].contiguous() for i in range(levels)]}


@pytest.mark.parametrize("dim", ["3d", "2d"])
@pytest.mark.parametrize("name", TR.VARIANTS)
def test_first_step_loss_is_the_loss_module_on_the_network_outputs(name, dim):
    tr = make_trainer(name, dim)
    tr.on_train_epoch_start()
    b = batch(dim, 5)
    outs = tr.network(b['data'].to(DEV))
    want = tr.loss(outs, [t.to(DEV) for t in b['target']]).detach().cpu().numpy()
    ref = float(TR.variant_loss(name, [o.detach().cpu() for o in outs], b['target']))
    assert len(outs) == len(b['target']) == len(tr.loss.weight_factors) and tr.loss.weight_factors[-1] > 0
    got = np.asarray(tr.train_step(b)["loss"])
    print(f"{name} {dim}: step loss {float(got):.7f} module {float(want):.7f} fp64 restatement {ref:.7f}")
    assert np.array_equal(got, want), (got, want)
    assert abs(float(got) - ref) <= 1e-5 * abs(ref), (float(got), ref)


@pytest.mark.parametrize("dim", ["3d", "2d"])
@pytest.mark.parametrize("name", TR.VARIANTS)
def test_graph_replays_equal_eager_steps_with_validation_in_between(name, dim):
    """eager: 5 train steps.  graphed: 1 eager warm-up step, the capture, 3 replays -- and a validation_step after the
    second and the fourth step.  Losses and every parameter agree bit for bit."""
    a, b = make_trainer(name, dim, graph=False), make_trainer(name, dim, graph=True)
    b.network.load_state_dict(a.network.state_dict())
    b.optimizer.fp.invalidate_packs()
    batches = [batch(dim, 30 + i) for i in range(5)]
    la = [np.asarray(a.train_step(x)["loss"]).copy() for x in batches]
    lb = []
    for i, x in enumerate(batches):
        lb.append(np.asarray(b.train_step(x)["loss"]).copy())
        if i in (1, 3):
            v = b.validation_step(batch(dim, 90 + i))
            assert np.isfinite(float(v['loss'])) and len(v['tp_hard']) == 3
    torch.cuda.synchronize()
    assert b._step_graph is not None and b._step_graph["graph"] is not None, "the step was never captured"
    for i, (x, y) in enumerate(zip(la, lb)):
        assert np.array_equal(x, y), f"loss of step {i}: eager {x} graph {y}"
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


@pytest.mark.parametrize("name", ["nnUNetTrainerTopk10LossMI355", "nnUNetTrainerDiceTopK10LossMI355"])
def test_bf16_network_precision_and_deep_supervision_off(name):
    """logits are fp32 under either network precision; with deep supervision switched off the network returns one tensor
    and the wrapped loss takes it as a one-level list"""
    tr = make_trainer(name, precision="bf16", base=32)     # (the bf16 conv engines take channels in blocks of 32)
    b = batch("3d", 6)
    l = float(tr.train_step(b)["loss"])
    assert np.isfinite(l) and l > 0
    tr.set_deep_supervision_enabled(False)
    out = tr.network(b['data'].to(DEV))
    assert torch.is_tensor(out) and out.dtype == torch.float32
    one = float(tr.loss.loss(out, b['target'][0].to(DEV)))
    ref = float(TR.variant_level_loss(name)(out.detach().cpu(), b['target'][0]))
    assert abs(one - ref) <= 1e-5 * abs(ref)
    tr.set_deep_supervision_enabled(True)


def _oracle_steps(name, dataset, heads, nlab, **kw):
    from oracle import step_oracle as SO, unet_oracle as UO
    tr = make_trainer(name, "3d", dataset)
    ora = UO.build_plainconv_unet(2, heads, 4, PLANS["3d"]["strides"], base=8, max_features=32, seed=0)
    tr.network.load_state_dict(ora.state_dict())
    tr.optimizer.fp.invalidate_packs()
    opt = SO.make_optimizer(ora.parameters())
    loss_fn = lambda outs, tgts: TR.variant_loss(name, outs, tgts, **kw)
    tr.on_train_epoch_start()
    for step in range(2):
        b = batch("3d", 10 + step, nlab)
        l_ref, _, _ = SO.train_step(ora, loss_fn, opt, b)
        l = float(tr.train_step(b)["loss"])
        lerr = abs(l - float(l_ref)) / abs(float(l_ref))
        ref_params = dict(ora.named_parameters())
        perr = max(float((p.detach().cpu() - ref_params[n].detach()).abs().max()) for n, p in tr.network.named_parameters())
        print(f"{name} step {step}: loss {l:.7f} oracle {float(l_ref):.7f} rel {lerr:.2e}; worst param err {perr:.2e}")
        assert lerr <= 1e-5, lerr
        assert perr <= 1e-5, perr


def test_ce_trainer_with_an_ignore_label_follows_the_oracle():
    _oracle_steps("nnUNetTrainerCELossMI355", IGNORE, 4, 5, ignore_label=4)


def test_dice_trainer_with_regions_follows_the_oracle():
    _oracle_steps("nnUNetTrainerDiceLossMI355", REGIONS_JSON, 3, 4, regions=REGIONS)


def test_topk_trainers_with_an_ignore_label_follow_the_oracle():
    _oracle_steps("nnUNetTrainerDiceTopK10LossMI355", IGNORE, 4, 5, ignore_label=4)
