"""CPU tests of the ResidualEncoderUNet surface: structure (the planner's two known answers, state_dict keys), the init
rule, the plans mapping, every refusal, the flat-parameter order.  No kernel runs here."""
import pytest
import torch
from torch import nn

import resenc_ref
from multimodal_mvd_seg_amd import network, trainer


def _kw(**over):
    kw = dict(conv_bias=True, norm_op=nn.InstanceNorm3d, norm_op_kwargs={'eps': 1e-5, 'affine': True}, dropout_op=None,
              dropout_op_kwargs=None, nonlin=nn.LeakyReLU, nonlin_kwargs={'inplace': True}, deep_supervision=True)
    kw.update(over)
    return kw


def _small(**over):
    args = dict(input_channels=resenc_ref.IN_CH, n_stages=3, features_per_stage=resenc_ref.FEATURES, conv_op=nn.Conv3d,
                kernel_sizes=3, strides=resenc_ref.STRIDES, n_blocks_per_stage=resenc_ref.BLOCKS,
                num_classes=resenc_ref.CLASSES, n_conv_per_stage_decoder=1)
    args.update(_kw())
    args.update(over)
    return network.MI355ResidualEncoderUNet(**args)


def test_feature_map_size_3d_is_the_planners_known_answer():
    # resencUNet_planner.py:38-44, its constructor arguments verbatim
    net = network.ResidualEncoderUNet(input_channels=1, n_stages=6, features_per_stage=(32, 64, 128, 256, 320, 320),
                                      conv_op=nn.Conv3d, kernel_sizes=3, strides=(1, 2, 2, 2, 2, 2),
                                      n_blocks_per_stage=(1, 3, 4, 6, 6, 6), num_classes=3,
                                      n_conv_per_stage_decoder=(1, 1, 1, 1, 1),
                                      conv_bias=True, norm_op=nn.InstanceNorm3d, norm_op_kwargs={}, dropout_op=None,
                                      nonlin=nn.LeakyReLU, nonlin_kwargs={'inplace': True}, deep_supervision=True)
    assert isinstance(net, network.MI355ResidualEncoderUNet)
    assert int(net.compute_conv_feature_map_size((128, 128, 128))) == 558319104


def test_feature_map_size_2d_is_the_planners_known_answer():
    # resencUNet_planner.py:47-53
    net = network.ResidualEncoderUNet(input_channels=1, n_stages=7, features_per_stage=(32, 64, 128, 256, 512, 512, 512),
                                      conv_op=nn.Conv2d, kernel_sizes=3, strides=(1, 2, 2, 2, 2, 2, 2),
                                      n_blocks_per_stage=(1, 3, 4, 6, 6, 6, 6), num_classes=3,
                                      n_conv_per_stage_decoder=(1, 1, 1, 1, 1, 1),
                                      conv_bias=True, norm_op=nn.InstanceNorm2d, norm_op_kwargs={}, dropout_op=None,
                                      nonlin=nn.LeakyReLU, nonlin_kwargs={'inplace': True}, deep_supervision=True)
    assert int(net.compute_conv_feature_map_size((512, 512))) == 129793792


def test_state_dict_keys_equal_the_torch_restatement():
    net, ref = _small(), resenc_ref.build()
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    for (k, v), w in zip(net.state_dict().items(), ref.state_dict().values()):
        assert tuple(v.shape) == tuple(w.shape), k
    keys = set(net.state_dict())
    assert "encoder.stem.convs.0.conv.weight" in keys
    assert "encoder.stages.0.blocks.0.conv2.norm.weight" in keys
    assert not any(k.startswith("encoder.stages.0.blocks.0.skip") for k in keys)          # identity skip: 32 -> 32, stride 1
    assert "encoder.stages.1.blocks.0.skip.1.conv.weight" in keys                         # pool, then projection
    assert "encoder.stages.1.blocks.0.skip.1.conv.bias" not in keys                       # (bias=False)
    assert "encoder.stages.1.blocks.0.skip.1.norm.bias" in keys
    assert "encoder.stages.1.blocks.1.conv1.all_modules.0.weight" in keys
    # strict interchange in both directions
    ref.load_state_dict(net.state_dict(), strict=True)
    net.load_state_dict(ref.state_dict(), strict=True)


def test_state_dict_keys_with_a_pool_only_skip():
    # equal channels across a strided stage (320 -> 320 in the planner's network): the skip is the pool alone, no keys
    feats, strides = [32, 64, 64], [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
    net = _small(features_per_stage=feats, strides=strides)
    ref = resenc_ref.build(features=feats, strides=strides)
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    blk = net.encoder.stages[2].blocks[0]
    assert len(blk.skip) == 1 and isinstance(blk.skip[0], nn.AvgPool3d) and not list(blk.skip.parameters())
    assert not any(k.startswith("encoder.stages.2.blocks.0.skip") for k in net.state_dict())
    # stride 1 with a channel change (a wider stem): the projection alone, at skip.0
    net = _small(stem_channels=16)
    assert "encoder.stages.0.blocks.0.skip.0.conv.weight" in net.state_dict()
    assert tuple(net.state_dict()["encoder.stages.0.blocks.0.skip.0.conv.weight"].shape) == (32, 16, 1, 1, 1)


def _resenc_plans(**kw):
    return trainer.make_plans(resenc_ref.PATCH, resenc_ref.STRIDES, batch_size=resenc_ref.BATCH,
                              unet_class_name='ResidualEncoderUNet', n_blocks_per_stage=resenc_ref.BLOCKS,
                              n_conv_per_stage_decoder=(1, 1), **kw)


def _from_plans(cls=None, plans=None):
    pm = trainer.PlansManager(plans or _resenc_plans())
    cfg = pm.get_configuration(next(iter(pm.plans['configurations'])))
    cls = cls or trainer.nnUNetTrainerMI355
    return cls.build_network_architecture(pm, resenc_ref.DATASET_JSON, cfg, resenc_ref.IN_CH, True)


def test_get_network_from_plans_maps_the_class_and_applies_both_inits():
    torch.manual_seed(0)
    net = _from_plans()
    assert isinstance(net, network.MI355ResidualEncoderUNet)
    assert [len(s.blocks) for s in net.encoder.stages] == list(resenc_ref.BLOCKS)
    assert [len(s.convs) for s in net.decoder.stages] == [1, 1]
    assert net.encoder.output_channels == resenc_ref.FEATURES
    assert list(net.state_dict().keys()) == list(resenc_ref.build().state_dict().keys())
    blocks = [m for m in net.modules() if isinstance(m, network.BasicBlockD)]
    assert len(blocks) == sum(resenc_ref.BLOCKS)
    for b in blocks:   # init_last_bn_before_add_to_0
        assert float(b.conv2.norm.weight.abs().max()) == 0 and float(b.conv2.norm.bias.abs().max()) == 0
        assert float(b.conv1.norm.weight.min()) == 1 and float(b.conv1.norm.bias.abs().max()) == 0
        if b._proj:
            assert float(b.skip[-1].norm.weight.min()) == 1          # only the norm in front of the add is zeroed
            assert b.skip[-1].conv.bias is None
    for m in net.modules():   # InitWeights_He(1e-2): conv biases at zero, weights drawn
        if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
            assert float(m.weight.std()) > 0 and (m.bias is None or float(m.bias.abs().max()) == 0)
    # the 2-D plan
    plans2 = trainer.make_plans((16, 16), [[1, 1], [2, 2], [2, 2]], configuration='2d', unet_class_name='ResidualEncoderUNet',
                                n_blocks_per_stage=(1, 2, 2), n_conv_per_stage_decoder=(1, 1))
    net2 = _from_plans(plans=plans2)
    assert isinstance(net2, network.MI355ResidualEncoderUNet) and net2.encoder.conv_op is nn.Conv2d
    assert isinstance(net2.encoder.stages[1].blocks[0].skip[0], nn.AvgPool2d)
    assert tuple(net2.state_dict()["encoder.stages.1.blocks.0.skip.1.conv.weight"].shape) == (64, 32, 1, 1)


def test_make_plans_defaults_are_unchanged():
    got = trainer.make_plans((32, 32, 32), [[1, 1, 1], [2, 2, 2]], batch_size=3, n_conv=2, spacing=(1, 2, 3))
    assert got == {'plans_name': 'nnUNetPlans', 'configurations': {'3d_fullres': {
        'patch_size': [32, 32, 32], 'batch_size': 3, 'UNet_class_name': 'PlainConvUNet', 'UNet_base_num_features': 32,
        'unet_max_num_features': 320, 'n_conv_per_stage_encoder': [2, 2], 'n_conv_per_stage_decoder': [2],
        'conv_kernel_sizes': [[3, 3, 3], [3, 3, 3]], 'pool_op_kernel_sizes': [[1, 1, 1], [2, 2, 2]], 'batch_dice': False,
        'spacing': [1.0, 2.0, 3.0]}}}
    cfg = _resenc_plans()['configurations']['3d_fullres']
    assert cfg['UNet_class_name'] == 'ResidualEncoderUNet'
    assert cfg['n_conv_per_stage_encoder'] == [1, 2, 2] and cfg['n_conv_per_stage_decoder'] == [1, 1]


def test_parameters_in_execution_order_is_a_permutation():
    net = _small()
    order = net.parameters_in_execution_order()
    assert len(order) == len(list(net.parameters())) == len({id(p) for p in order})
    assert {id(p) for p in order} == {id(p) for p in net.parameters()}
    names = {id(p): n for n, p in net.named_parameters()}
    seq = [names[id(p)] for p in order]
    assert seq[0].startswith("encoder.stem.")
    first = {pre: min(i for i, n in enumerate(seq) if n.startswith(pre))
             for pre in ("encoder.stem.", "encoder.stages.0.", "encoder.stages.2.", "decoder.transpconvs.0.", "decoder.stages.0.",
                         "decoder.seg_layers.0.", "decoder.transpconvs.1.")}
    assert sorted(first, key=first.get) == list(first)


@pytest.mark.parametrize("over,what", [
    (dict(norm_op=nn.BatchNorm3d), "BatchNorm"),
    (dict(block=nn.Identity), "block"),
    (dict(bottleneck_channels=16), "bottleneck_channels"),
    (dict(bottleneck_channels=[None, 16, 16]), "bottleneck_channels"),
    (dict(dropout_op=nn.Dropout3d, dropout_op_kwargs={'p': 0.1}), "dropout"),
    (dict(nonlin_first=True), "nonlin_first"),
    (dict(pool='max'), "pool"),
])
def test_constructor_refusals_name_the_class(over, what):
    with pytest.raises(NotImplementedError, match="ResidualEncoderUNet") as e:
        _small(**over)
    assert what.lower() in str(e.value).lower()


def test_block_refuses_stochastic_depth_and_squeeze_excitation():
    args = (nn.Conv3d, 32, 32, 3, 1, True, nn.InstanceNorm3d, None, None, None, nn.LeakyReLU, None)
    network.BasicBlockD(*args)
    with pytest.raises(NotImplementedError, match="ResidualEncoderUNet.*stochastic depth"):
        network.BasicBlockD(*args, stochastic_depth_p=0.1)
    with pytest.raises(NotImplementedError, match="ResidualEncoderUNet.*squeeze"):
        network.BasicBlockD(*args, squeeze_excitation=True)
    with pytest.raises(NotImplementedError, match="ResidualEncoderUNet.*squeeze"):
        network.StackedResidualBlocks(2, *args, squeeze_excitation=True)


def test_bf16_cpu_input_and_the_other_trainers_are_refused():
    net = _small()
    with pytest.raises(NotImplementedError, match="ResidualEncoderUNet"):
        network.set_precision(net, 'bf16')
    network.set_precision(net, 'fp32')
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.zeros(1, resenc_ref.IN_CH, 16, 16, 16))
    for cls in (trainer.ContrastiveTrainerMI355, trainer.FinalNetTrainerMI355, trainer.nnUNetTrainerBNMI355):
        with pytest.raises(NotImplementedError, match="ResidualEncoderUNet"):
            _from_plans(cls)
    # the InstanceNorm subclasses build it through the parent's builder
    assert isinstance(_from_plans(trainer.nnUNetTrainerAdamMI355), network.MI355ResidualEncoderUNet)
