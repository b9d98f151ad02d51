"""CPU tests of the BatchNorm3d networks (nnUNetTrainerBN.py:31-32): construction, the reference's state_dict keys, the
trainer variant's builder, every refusal with its message, and the conditioning of the shared oracle reference that the
GPU tests (tests/test_gpu_batchnorm.py) are held to.  No kernel runs here."""
import types

import pytest
import torch
from torch import nn

import bn_ref


def _net(norm_op=nn.BatchNorm3d, kwargs=None, ds=True):
    from multimodal_mvd_seg_amd import network
    return network.MI355PlainConvUNet(bn_ref.IN_CH, 3, bn_ref.FEATURES, nn.Conv3d, 3, bn_ref.STRIDES, 2, bn_ref.CLASSES, 2,
                                      True, norm_op, kwargs or {'eps': 1e-5, 'affine': True}, None, None, nn.LeakyReLU,
                                      {'inplace': True}, deep_supervision=ds)


def test_bn_network_constructs_with_the_reference_state_dict():
    from multimodal_mvd_seg_amd import network
    net = _net()
    blocks = [m for m in net.modules() if isinstance(m, network.ConvDropoutNormReLU)]
    assert len(blocks) == 10 and all(isinstance(b.norm, network.HipBatchNorm3d) and b.batch_norm for b in blocks)
    assert all(isinstance(b.all_modules[1], nn.BatchNorm3d) for b in blocks)
    ora = bn_ref.bn_oracle()
    sd, ref = net.state_dict(), ora.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype, k
    for suffix in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        assert f"encoder.stages.0.0.convs.0.norm.{suffix}" in sd and f"decoder.stages.1.convs.1.all_modules.1.{suffix}" in sd
    # interchange, both directions, strict
    net.load_state_dict(ref, strict=True)
    ora.load_state_dict(net.state_dict(), strict=True)
    k = "encoder.stages.1.0.convs.0.norm.running_var"
    assert torch.equal(net.state_dict()[k], ref[k]) and not torch.equal(ref[k], torch.ones_like(ref[k]))


def test_bn_buffers_are_module_buffers_not_flat_parameters():
    net = _net()
    names = {n for n, _ in net.named_parameters()}
    assert not any("running_" in n or "num_batches_tracked" in n for n in names)
    bufs = dict(net.named_buffers())
    assert bufs["encoder.stages.0.0.convs.0.norm.num_batches_tracked"].dtype == torch.int64
    assert bufs["encoder.stages.0.0.convs.0.norm.running_mean"].dtype == torch.float32


def test_trainer_variant_builds_a_bn_network_from_plans():
    import multimodal_mvd_seg_amd as pkg
    from multimodal_mvd_seg_amd import network, trainer
    assert pkg.nnUNetTrainerBNMI355 is trainer.nnUNetTrainerBNMI355
    assert issubclass(trainer.nnUNetTrainerBNMI355, trainer.nnUNetTrainerMI355)
    # only the static builder is overridden, as in the reference's class
    own = {k for k in vars(trainer.nnUNetTrainerBNMI355) if not k.startswith("__")}
    assert own == {"build_network_architecture"}
    plans = trainer.make_plans(bn_ref.PATCH, bn_ref.STRIDES, batch_size=bn_ref.BATCH)
    pm = trainer.PlansManager(plans)
    net = trainer.nnUNetTrainerBNMI355.build_network_architecture(pm, bn_ref.DATASET_JSON, pm.get_configuration("3d_fullres"),
                                                                  bn_ref.IN_CH, True)
    assert isinstance(net, network.MI355PlainConvUNet)
    assert list(net.state_dict().keys()) == list(bn_ref.bn_oracle().state_dict().keys())
    norms = [m for m in net.modules() if isinstance(m, network.HipBatchNorm3d)]
    assert norms and all(m.eps == 1e-5 and m.momentum == 0.1 and m.affine and m.track_running_stats for m in norms)
    # the default of get_network_from_plans and the dual-branch builder stay on InstanceNorm
    base = trainer.nnUNetTrainerMI355.build_network_architecture(pm, bn_ref.DATASET_JSON, pm.get_configuration("3d_fullres"),
                                                                 bn_ref.IN_CH, True)
    assert not any(isinstance(m, nn.BatchNorm3d) for m in base.modules())
    dual = trainer.ContrastiveTrainerMI355.build_network_architecture(pm, bn_ref.DATASET_JSON,
                                                                      pm.get_configuration("3d_fullres"), bn_ref.IN_CH, True)
    assert not any(isinstance(m, nn.BatchNorm3d) for m in dual.modules())


def test_residual_encoder_stays_refused():
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(bn_ref.PATCH, bn_ref.STRIDES)
    plans['configurations']['3d_fullres']['UNet_class_name'] = 'ResidualEncoderUNet'
    pm = trainer.PlansManager(plans)
    with pytest.raises(NotImplementedError, match="ResidualEncoderUNet"):
        trainer.nnUNetTrainerBNMI355.build_network_architecture(pm, bn_ref.DATASET_JSON, pm.get_configuration("3d_fullres"),
                                                                bn_ref.IN_CH, True)


def test_instancenorm_state_dict_keys_are_unchanged():
    from oracle import unet_oracle as UO
    net = _net(nn.InstanceNorm3d)
    ora = UO.build_plainconv_unet(bn_ref.IN_CH, bn_ref.CLASSES, 3, bn_ref.STRIDES, features_per_stage=bn_ref.FEATURES)
    assert list(net.state_dict().keys()) == list(ora.state_dict().keys())
    assert not any("running_" in k or "num_batches_tracked" in k for k in net.state_dict())
    from multimodal_mvd_seg_amd import network
    assert all(not b.batch_norm and type(b.norm) is network.HipInstanceNorm3d
               for b in net.modules() if isinstance(b, network.ConvDropoutNormReLU))


@pytest.mark.parametrize("kwargs,msg", [
    ({'eps': 1e-5, 'affine': True, 'momentum': None}, r"momentum=None"),
    ({'eps': 1e-5, 'affine': True, 'track_running_stats': False}, r"track_running_stats=False"),
    ({'eps': 1e-5, 'affine': False}, r"BatchNorm3d\(affine=False\)"),
])
def test_unsupported_batchnorm_settings_are_refused_with_a_message(kwargs, msg):
    with pytest.raises(NotImplementedError, match=msg):
        _net(kwargs=kwargs)
    from multimodal_mvd_seg_amd import network
    direct = {k: v for k, v in kwargs.items()}
    with pytest.raises(NotImplementedError, match=msg):
        network.HipBatchNorm3d(8, **direct)


def test_the_bn_block_is_its_own_class_and_the_instancenorm_block_keeps_refusing_batchnorm():
    from multimodal_mvd_seg_amd import network
    kw = dict(norm_op=nn.BatchNorm3d, norm_op_kwargs={'eps': 1e-5, 'affine': True}, nonlin=nn.LeakyReLU,
              nonlin_kwargs={'inplace': True})
    blk = network.ConvDropoutBatchNormReLU(nn.Conv3d, 4, 8, 3, 1, True, **kw)
    assert isinstance(blk, network.ConvDropoutNormReLU) and blk.batch_norm and isinstance(blk.norm, network.HipBatchNorm3d)
    with pytest.raises(NotImplementedError, match="only nn.InstanceNorm3d"):
        network.ConvDropoutNormReLU(nn.Conv3d, 4, 8, 3, 1, True, **kw)
    with pytest.raises(NotImplementedError, match="only nn.BatchNorm3d"):
        network.ConvDropoutBatchNormReLU(nn.Conv3d, 4, 8, 3, 1, True, **{**kw, "norm_op": nn.InstanceNorm3d})
    st = network.StackedConvBlocks(2, nn.Conv3d, 4, 8, 3, 1, True, **kw)
    assert all(type(b) is network.ConvDropoutBatchNormReLU for b in st.convs)


def test_other_norms_stay_refused():
    with pytest.raises(NotImplementedError, match="norm_op"):
        _net(nn.GroupNorm)
    with pytest.raises(NotImplementedError, match="norm_op"):
        _net(nn.BatchNorm2d)


def test_one_value_per_channel_in_training_is_refused_as_torch_refuses_it():
    from multimodal_mvd_seg_amd import network
    bn = network.HipBatchNorm3d(8)
    x = torch.zeros(1, 8, 1, 1, 1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        bn(x)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        nn.BatchNorm3d(8)(x)           # torch's own refusal, same words
    bn.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # eval takes M == 1; it then needs the device
        bn(x)


def test_backward_through_an_eval_forward_is_refused():
    from multimodal_mvd_seg_amd import ops
    ctx = types.SimpleNamespace(training=False)
    with pytest.raises(RuntimeError, match="backward through an eval-mode forward"):
        ops.BatchNormLeakyReLUFn.backward(ctx, torch.zeros(1, 8, 2, 2, 2))


def test_set_precision_reaches_bn_blocks():
    from multimodal_mvd_seg_amd import network
    net = network.set_precision(_net(), "bf16")
    assert all(b.precision == "bf16" for b in net.modules() if isinstance(b, network.ConvDropoutNormReLU))
    assert all(b.dtype == torch.float32 for n, b in net.named_buffers() if "running_" in n)


def test_bn_blocks_never_enter_an_instancenorm_fusion():
    from multimodal_mvd_seg_amd import network
    net = network.set_precision(_net(), "bf16")
    st = net.decoder.stages[-1]
    blk, nxt = st.convs[0], st.convs[1]
    inp = torch.zeros(2, 64, 16, 16, 16)       # never touched: the answer comes before any shape query
    assert network.StackedConvBlocks._can_fuse(blk, nxt, inp) is False


def test_shared_reference_is_well_conditioned():
    """The GPU network test compares fp32 kernels with the fp64 oracle at fixed bars (logits 1e-4, loss 1e-5, gradients at
    the tiny-U-Net bars, parameters after 1 and 3 steps 1e-5, running buffers 2e-6 relative).  torch's own fp32 evaluation
    of the same network must stay within a quarter of each bar, or the seed / input scale is badly conditioned."""
    r64, r32 = bn_ref.reference64(), bn_ref.evaluate(torch.float32)
    for a, b in zip(r32['logits'], r64['logits']):
        assert float((a.double() - b).abs().max()) <= 0.25 * 1e-4
    for a, b in zip(r32['losses'], r64['losses']):
        assert abs(a - b) <= 0.25 * 1e-5 * max(1.0, abs(b))
    for n, g in r64['grads'].items():
        assert float((r32['grads'][n].double() - g).abs().max()) <= 0.25 * bn_ref.grad_tol(n, g), n
    for step in (1, 3):
        for n, p in r64['params'][step].items():
            assert float((r32['params'][step][n].double() - p).abs().max()) <= 0.25 * 1e-5, (step, n)
        for n, v in r64['buffers'][step].items():
            if v.dtype.is_floating_point:
                err = float((r32['buffers'][step][n].double() - v).abs().max())
                assert err <= 0.25 * bn_ref.buffer_tol(v), (step, n, err)
            else:
                assert int(v) == step
