"""Host-side mirror of the reference's trainer plugin surface for the train-step hot path.

`nnUNetTrainerMI355` keeps the signatures the reference discovers and calls by name
(nnUNet/nnunetv2/training/nnUNetTrainer/nnUNetTrainer.py): `__init__(plans, configuration, fold, dataset_json,
unpack_dataset, device, specified_cfg)` :69-70, `initialize` :201-228, static `build_network_architecture`
:268-294, `_get_deep_supervision_scales` :296-302, `_set_batch_size_and_oversample` :304-349, `_build_loss`
:351-375, `configure_optimizers` :473-477, `set_deep_supervision_enabled` :802-810, `train_step` :888-925,
`validation_step` :942-1004, `on_validation_epoch_end` :1006-1037.  In the reference tree this class would derive
from nnUNetTrainer and only override `build_network_architecture` / `_build_loss` / `configure_optimizers` /
`initialize`; upstream nnunetv2 cannot be imported here (batchgenerators & co. absent), so the
step-relevant parts of the base class are restated.  Data loading, logging, checkpoint files and final validation
are out of scope.

`ContrastiveTrainerMI355` mirrors the dual-branch mutual-distillation step
(nnUNet/nnunetv2/training/nnUNetTrainer/MVDTrainer.py:879-925; lambdas :132-134).
"""
import os

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from . import losses, ops
from .dataloading import DeviceDataLoader2D, DeviceDataLoader3D, get_patch_size
from .network import (InitWeights_He, MI355PlainConvUNet, MI355ResidualEncoderUNet, MVDDualBranchNet,
                      get_finalnet_from_plans, init_last_bn_before_add_to_0, set_precision)
from .optim import CosineAnnealingLR, FlatParams, FusedAdam, FusedSGDNesterov, PolyLRScheduler
from .parallel import BucketedGradReducer, broadcast_parameters, ddp_batch_split


ANISO_THRESHOLD = 3  # configuration.py:7


# ------------------------------------------------------------------------------------------------ plans (input contract)
class ConfigurationManager:
    """The plans.json keys the builder reads (get_network_from_plans.py:26-83; plans_handler.py:32-178)."""

    def __init__(self, configuration_dict: dict):
        self.configuration = configuration_dict

    def __getattr__(self, k):
        cfg = self.__dict__.get('configuration', {})
        if k in cfg:
            return cfg[k]
        raise AttributeError(k)

    # plans_handler.py:68-69, :139-148 -- what the segmentation export reads (export.py)
    @property
    def spacing(self):
        if 'spacing' not in self.configuration:
            raise AttributeError("the configuration has no 'spacing' (needed to export a prediction)")
        return self.configuration['spacing']

    @property
    def resampling_fn_probabilities_kwargs(self):
        # the default plans' values (experiment_planning/experiment_planners/default_experiment_planner.py)
        kw = {'is_seg': False, 'order': 1, 'order_z': 0, 'force_separate_z': None}
        kw.update(self.configuration.get('resampling_fn_probabilities_kwargs', {}))
        return kw

    @property
    def resampling_fn_probabilities(self):
        from functools import partial
        from . import export
        name = self.configuration.get('resampling_fn_probabilities', 'resample_data_or_seg_to_shape')
        if name != 'resample_data_or_seg_to_shape':
            raise NotImplementedError(f"resampling_fn_probabilities '{name}': only resample_data_or_seg_to_shape")
        return partial(export.resample_data_or_seg_to_shape, **self.resampling_fn_probabilities_kwargs)


class LabelManager:
    """label_handling.py:21-234: plain labels, overlapping regions (sigmoid heads, `regions_class_order`) and the ignore
    label.  The inference nonlinearity is not held here: export.py takes the regions branch from `has_regions`."""

    def __init__(self, label_dict: dict, regions_class_order=None, force_use_labels: bool = False):
        self._sanity_check(label_dict)
        self.label_dict = label_dict
        self.regions_class_order = regions_class_order
        self._force_use_labels = force_use_labels
        self._has_regions = False if force_use_labels else any(
            isinstance(i, (tuple, list)) and len(i) > 1 for i in label_dict.values())
        self._ignore_label = self._determine_ignore_label()
        self._all_labels = self._get_all_labels()
        self._regions = self._get_regions()
        if self.has_ignore_label:
            assert self.ignore_label == max(self.all_labels) + 1, \
                'If you use the ignore label it must have the highest label value! It cannot be 0 or in between other ' \
                'labels.'

    @staticmethod
    def _sanity_check(label_dict: dict):
        if 'background' not in label_dict.keys():
            raise RuntimeError('Background label not declared (remember that this should be label 0!)')
        bg_label = label_dict['background']
        if isinstance(bg_label, (tuple, list)):
            raise RuntimeError(f"Background label must be 0. Not a list. Not a tuple. Your background label: {bg_label}")
        assert int(bg_label) == 0, f"Background label must be 0. Your background label: {bg_label}"

    def _get_all_labels(self):
        all_labels = []
        for k, r in self.label_dict.items():
            if k == 'ignore':
                continue
            if isinstance(r, (tuple, list)):
                all_labels += [int(ri) for ri in r]
            else:
                all_labels.append(int(r))
        return sorted(set(all_labels))

    def _get_regions(self):
        if not self._has_regions or self._force_use_labels:
            return None
        assert self.regions_class_order is not None, \
            'if region-based training is requested then you need to define regions_class_order!'
        regions = []
        for k, r in self.label_dict.items():
            if k == 'ignore':
                continue
            if (np.isscalar(r) and r == 0) or \
                    (isinstance(r, (tuple, list)) and len(np.unique(r)) == 1 and np.unique(r)[0] == 0):
                continue  # regions that are background
            regions.append(tuple(r) if isinstance(r, list) else r)
        assert len(self.regions_class_order) == len(regions), \
            'regions_class_order must have as many entries as there are regions'
        return regions

    def _determine_ignore_label(self):
        ignore_label = self.label_dict.get('ignore')
        if ignore_label is not None:
            assert isinstance(ignore_label, int), \
                f'Ignore label has to be an integer. It cannot be a region (list/tuple). Got {type(ignore_label)}.'
        return ignore_label

    @property
    def has_regions(self) -> bool:
        return self._has_regions

    @property
    def has_ignore_label(self) -> bool:
        return self.ignore_label is not None

    @property
    def all_regions(self):
        return self._regions

    @property
    def all_labels(self):
        return self._all_labels

    @property
    def ignore_label(self):
        return self._ignore_label

    @staticmethod
    def filter_background(classes_or_regions):
        return [i for i in classes_or_regions if
                ((not isinstance(i, (tuple, list))) and i != 0) or
                (isinstance(i, (tuple, list)) and not (len(np.unique(i)) == 1 and np.unique(i)[0] == 0))]

    @property
    def foreground_regions(self):
        return self.filter_background(self.all_regions)

    @property
    def foreground_labels(self):
        return self.filter_background(self.all_labels)

    @property
    def num_segmentation_heads(self):
        return len(self.foreground_regions) if self.has_regions else len(self.all_labels)


class PlansManager:
    def __init__(self, plans: dict):
        self.plans = plans

    def get_configuration(self, name):
        cfgs = self.plans['configurations']
        cfg = dict(cfgs[name])
        if 'inherits_from' in cfg:  # plans_handler.py:197-219
            base = dict(self.get_configuration(cfg['inherits_from']).configuration)
            base.update(cfg)
            cfg = base
        return ConfigurationManager(cfg)

    def get_label_manager(self, dataset_json):
        return LabelManager(dataset_json['labels'], regions_class_order=dataset_json.get('regions_class_order'))

    # plans_handler.py:252-257; plans without the keys keep the axis order
    @property
    def transpose_forward(self):
        return list(self.plans.get('transpose_forward', [0, 1, 2]))

    @property
    def transpose_backward(self):
        return list(self.plans.get('transpose_backward', [0, 1, 2]))


def determine_num_input_channels(plans_manager, configuration_manager, dataset_json):
    """label_handling.py:283-301: the modalities, plus one one-hot channel per foreground label of the previous stage's
    segmentation for a cascaded configuration (previous_stage_name set, :294-297)."""
    key = 'channel_names' if 'channel_names' in dataset_json else 'modality'
    num_modalities = len(dataset_json[key])
    if getattr(configuration_manager, 'previous_stage_name', None) is not None:
        return num_modalities + len(plans_manager.get_label_manager(dataset_json).foreground_labels)
    return num_modalities


def make_plans(patch_size, strides, batch_size=2, base_features=32, max_features=320, n_conv=2, batch_dice=False,
               conv_kernel_sizes=None, configuration='3d_fullres', spacing=None, previous_stage_name=None,
               next_stage_names=None, cascade_configuration=None, cascade_spacing=None, unet_class_name='PlainConvUNet',
               n_blocks_per_stage=None, n_conv_per_stage_decoder=None):
    """A minimal nnUNetPlans.json-shaped dict for the synthetic configurations of BASELINE.json.  `configuration`: the name
    of the entry ('2d' with a 2-tuple patch size and 2-tuple strides writes a 2-D plan).  spacing / previous_stage_name /
    next_stage_names are written into the entry when given.  cascade_configuration names a second entry that inherits
    from the first (`inherits_from`, as the planner writes 3d_cascade_fullres), has it as its previous stage and is
    listed as its next stage: a two-stage plan.  unet_class_name 'ResidualEncoderUNet' with n_blocks_per_stage (written as
    n_conv_per_stage_encoder, the key the ResEnc planner uses for its block counts) and n_conv_per_stage_decoder writes a
    residual-encoder plan; left at None both keep [n_conv] per stage."""
    n = len(strides)
    enc = [n_conv] * n if n_blocks_per_stage is None else [int(b) for b in n_blocks_per_stage]
    dec = [n_conv] * (n - 1) if n_conv_per_stage_decoder is None else [int(b) for b in n_conv_per_stage_decoder]
    if len(enc) != n or len(dec) != n - 1:
        raise ValueError(f"n_blocks_per_stage needs {n} entries and n_conv_per_stage_decoder {n - 1}")
    cfg = {
        'patch_size': list(patch_size), 'batch_size': batch_size, 'UNet_class_name': unet_class_name,
        'UNet_base_num_features': base_features, 'unet_max_num_features': max_features,
        'n_conv_per_stage_encoder': enc, 'n_conv_per_stage_decoder': dec,
        'conv_kernel_sizes': conv_kernel_sizes or [[3] * len(patch_size)] * n,
        'pool_op_kernel_sizes': [list(s) for s in strides],
        'batch_dice': batch_dice}
    if spacing is not None:
        cfg['spacing'] = [float(v) for v in spacing]
    if previous_stage_name is not None:
        cfg['previous_stage_name'] = previous_stage_name
    if next_stage_names is not None:
        cfg['next_stage_names'] = list(next_stage_names)
    configurations = {configuration: cfg}
    if cascade_configuration is not None:
        cfg['next_stage_names'] = list(cfg.get('next_stage_names', [])) + [cascade_configuration]
        # the inherited next_stage_names is overwritten: the last stage has none
        second = {'inherits_from': configuration, 'previous_stage_name': configuration, 'next_stage_names': None}
        if cascade_spacing is not None:
            second['spacing'] = [float(v) for v in cascade_spacing]
        configurations[cascade_configuration] = second
    return {'plans_name': 'nnUNetPlans', 'configurations': configurations}


def get_network_from_plans(plans_manager, dataset_json, configuration_manager, num_input_channels,
                           deep_supervision=True, norm_op=nn.InstanceNorm3d, norm_op_kwargs=None):
    """get_network_from_plans.py:15-92: 'PlainConvUNet', and 'ResidualEncoderUNet' (:36, :46-52, :61-65, :90-91) with
    n_blocks_per_stage = n_conv_per_stage_encoder and the second init pass.  norm_op / norm_op_kwargs: what the
    network_architecture trainer variants replace (nnUNetTrainerBN.py:31-32); the default is the builder's own.
    dim = len(conv_kernel_sizes[0]) picks the conv (:21-23): 3 -> nn.Conv3d, 2 -> nn.Conv2d (the 2d configuration) with the
    norm of the same family in two dimensions (InstanceNorm2d; get_matching_batchnorm for the BN variant)."""
    num_stages = len(configuration_manager.conv_kernel_sizes)
    dim = len(configuration_manager.conv_kernel_sizes[0])
    if dim not in (2, 3):
        raise NotImplementedError(f"{dim}-D plans: the 3d_fullres and 2d configurations are built")
    conv_op = nn.Conv3d if dim == 3 else nn.Conv2d
    if dim == 2:
        norm_op = {nn.InstanceNorm3d: nn.InstanceNorm2d, nn.BatchNorm3d: nn.BatchNorm2d}.get(norm_op, norm_op)
    name = configuration_manager.UNet_class_name
    if name not in ('PlainConvUNet', 'ResidualEncoderUNet'):
        raise NotImplementedError(f"UNet_class_name {name!r}: PlainConvUNet and ResidualEncoderUNet are built")
    residual = name == 'ResidualEncoderUNet'
    label_manager = plans_manager.get_label_manager(dataset_json)
    blocks = {'n_blocks_per_stage' if residual else 'n_conv_per_stage': configuration_manager.n_conv_per_stage_encoder}
    model = (MI355ResidualEncoderUNet if residual else MI355PlainConvUNet)(
        input_channels=num_input_channels, n_stages=num_stages,
        features_per_stage=[min(configuration_manager.UNet_base_num_features * 2 ** i,
                                configuration_manager.unet_max_num_features) for i in range(num_stages)],
        conv_op=conv_op, kernel_sizes=configuration_manager.conv_kernel_sizes,
        strides=configuration_manager.pool_op_kernel_sizes, num_classes=label_manager.num_segmentation_heads,
        deep_supervision=deep_supervision, **blocks,
        n_conv_per_stage_decoder=configuration_manager.n_conv_per_stage_decoder, conv_bias=True,
        norm_op=norm_op, norm_op_kwargs=dict(norm_op_kwargs or {'eps': 1e-5, 'affine': True}), dropout_op=None,
        dropout_op_kwargs=None, nonlin=nn.LeakyReLU, nonlin_kwargs={'inplace': True})
    model.apply(InitWeights_He(1e-2))
    if residual:
        model.apply(init_last_bn_before_add_to_0)   # (:90-91)
    return model


def _refuse_residual_plans(configuration_manager, who):
    if getattr(configuration_manager, 'UNet_class_name', 'PlainConvUNet') == 'ResidualEncoderUNet':
        raise NotImplementedError(f"{who}: ResidualEncoderUNet plans are built for the single-network InstanceNorm trainers "
                                  f"only")


# ------------------------------------------------------------------------------------------------ trainer
class nnUNetTrainerMI355(object):
    def __init__(self, plans: dict, configuration: str, fold: int, dataset_json: dict, unpack_dataset: bool = True,
                 device: torch.device = torch.device('cuda'), specified_cfg: str = ''):
        self.is_ddp = dist.is_available() and dist.is_initialized()
        self.local_rank = 0 if not self.is_ddp else dist.get_rank()
        self.device = device
        if self.device.type != 'cuda':
            raise RuntimeError("nnUNetTrainerMI355 needs an MI355X (device type 'cuda'); there is no CPU path")
        self.plans_manager = PlansManager(plans)
        self.configuration_manager = self.plans_manager.get_configuration(configuration)
        self.configuration_name = configuration
        self.dataset_json = dataset_json
        self.fold = fold
        self.unpack_dataset = unpack_dataset
        self.specified_cfg = specified_cfg
        # nnUNetTrainer.py:143-149
        self.initial_lr = 1e-2
        self.weight_decay = 3e-5
        self.oversample_foreground_percent = 0.33
        self.num_iterations_per_epoch = 250
        self.num_val_iterations_per_epoch = 50
        self.num_epochs = 200
        self.current_epoch = 0
        self.enable_deep_supervision = True
        self.label_manager = self.plans_manager.get_label_manager(dataset_json)
        self.num_input_channels = None
        self.network = None
        self.optimizer = self.lr_scheduler = None
        self.grad_scaler = None  # fp32 path (the reference's CPU branch: no autocast, no GradScaler, :906,:921-924)
        # "bf16": the reference's autocast path (:906) restated for MI355X -- bf16 activations on the bf16 MFMA engine,
        # fp32 master weights / statistics / losses / optimizer, no GradScaler (network.set_precision)
        self.precision = 'fp32'
        self.loss = None
        self.reducer = None
        self.ddp_bucket_bytes = 25 * 1024 * 1024  # DDP's default bucket_cap_mb (nnUNetTrainer.py:222 passes none)
        self.was_initialized = False
        self.batch_size = None
        # train_step replayed as one hipGraph launch after `hip_graph_warmup` eager steps (MVD_HIPGRAPH=0: always eager)
        self.use_hip_graph = os.environ.get("MVD_HIPGRAPH", "1") != "0"
        self.hip_graph_warmup = 3
        self._step_graph = None

    # -- plugin surface -------------------------------------------------------------------------------------
    @staticmethod
    def build_network_architecture(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                   enable_deep_supervision: bool = True) -> nn.Module:
        return get_network_from_plans(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                      deep_supervision=enable_deep_supervision)

    def initialize(self):
        if self.was_initialized:
            raise RuntimeError("You have called self.initialize even though the trainer was already initialized. "
                               "That should not happen.")
        self.num_input_channels = determine_num_input_channels(self.plans_manager, self.configuration_manager,
                                                               self.dataset_json)
        self.network = self.build_network_architecture(self.plans_manager, self.dataset_json,
                                                       self.configuration_manager, self.num_input_channels,
                                                       self.enable_deep_supervision).to(self.device)
        set_precision(self.network, self.precision)
        self.optimizer, self.lr_scheduler = self.configure_optimizers()
        if self.use_hip_graph:
            self.optimizer.fp.pack16_inplace = True   # the captured repack rewrites the buffers the captured forward reads
        if self.is_ddp:
            # DDP(network): broadcast rank 0's weights, then reduce gradients bucket-wise during backward (:220-222)
            broadcast_parameters(self.optimizer.fp)
            self.reducer = BucketedGradReducer(self.optimizer.fp, self.ddp_bucket_bytes, optimizer=self.optimizer)
        self.loss = self._build_loss()
        self._set_batch_size_and_oversample()
        self.was_initialized = True

    def _flat_params(self):
        # flat buffers in forward-execution order (network.parameters_in_execution_order): the gradient all-reduce buckets --
        # contiguous slices cut from the end -- then complete in backward order (parallel.BucketedGradReducer)
        order = getattr(self.network, "parameters_in_execution_order", None)
        params = order() if order is not None else list(self.network.parameters())
        name_of = {id(p): n for n, p in self.network.named_parameters()}   # (the layout signature of the optimizer state)
        return FlatParams([(name_of.get(id(p)), p) for p in params])

    def configure_optimizers(self):
        optimizer = FusedSGDNesterov(self._flat_params(), self.initial_lr,
                                     weight_decay=self.weight_decay, momentum=0.99, nesterov=True, max_grad_norm=12)
        lr_scheduler = PolyLRScheduler(optimizer, self.initial_lr, self.num_epochs)
        return optimizer, lr_scheduler

    def _get_deep_supervision_scales(self):
        if self.enable_deep_supervision:
            return list(list(i) for i in 1 / np.cumprod(np.vstack(
                self.configuration_manager.pool_op_kernel_sizes), axis=0))[:-1]
        return None

    def _set_batch_size_and_oversample(self):
        if not self.is_ddp:
            self.batch_size = self.configuration_manager.batch_size
        else:
            bs, ov = ddp_batch_split(self.configuration_manager.batch_size, dist.get_world_size(),
                                     self.oversample_foreground_percent)
            self.batch_size = bs[dist.get_rank()]
            self.oversample_foreground_percent = ov[dist.get_rank()]

    @property
    def is_cascaded(self) -> bool:
        """nnUNetTrainer.py:135-140."""
        return getattr(self.configuration_manager, 'previous_stage_name', None) is not None

    def _check_cascade(self):
        """The cascade is built for plain labels without an ignore label in a 3-D configuration."""
        if not self.is_cascaded:
            return
        if self.label_manager.has_regions:
            raise NotImplementedError("cascade configurations (previous_stage_name) with region-based labels are not built: "
                                      "the cascade stage one-hot encodes plain labels")
        if self.label_manager.has_ignore_label:
            raise NotImplementedError("cascade configurations (previous_stage_name) with an ignore label are not built")
        if len(self.configuration_manager.patch_size) != 3:
            raise NotImplementedError("cascade configurations (previous_stage_name) need a 3-D plan: nnU-Net plans no 2-D "
                                      "cascade")
        if len(self.label_manager.foreground_labels) > 8:
            raise NotImplementedError(f"cascade configurations with {len(self.label_manager.foreground_labels)} foreground "
                                      f"labels: the cascade stage of the feed holds at most 8")

    def _build_loss(self):
        self._check_cascade()
        if (self.label_manager.has_regions or self.label_manager.has_ignore_label) and \
                self.label_manager.num_segmentation_heads > ops.REGION_KMAX:
            # the limit is the loss kernels'; a network with more heads can still be built for inference and export, and
            # the plain-label loss keeps refusing in mvd_dcce_fwd as before
            raise NotImplementedError(f"{self.label_manager.num_segmentation_heads} segmentation heads: the fused loss "
                                      f"kernels hold at most {ops.REGION_KMAX}")
        if self.label_manager.has_regions:
            # (:352-357) the targets stay the feed's float label map: the loss converts label -> regions per voxel, which
            # commutes with the order-0 deep-supervision resize
            loss = losses.DC_and_BCE_loss({}, {'batch_dice': self.configuration_manager.batch_dice, 'do_bg': True,
                                               'smooth': 1e-5, 'ddp': self.is_ddp},
                                          use_ignore_label=self.label_manager.ignore_label is not None,
                                          dice_class=losses.MemoryEfficientSoftDiceLoss,
                                          regions=self.label_manager.foreground_regions,
                                          ignore_label=self.label_manager.ignore_label)
        else:
            loss = losses.DC_and_CE_loss({'batch_dice': self.configuration_manager.batch_dice, 'smooth': 1e-5,
                                          'do_bg': False, 'ddp': self.is_ddp}, {}, weight_ce=1, weight_dice=1,
                                         ignore_label=self.label_manager.ignore_label,
                                         dice_class=losses.MemoryEfficientSoftDiceLoss)
        if self.enable_deep_supervision:
            deep_supervision_scales = self._get_deep_supervision_scales()
            weights = np.array([1 / (2 ** i) for i in range(len(deep_supervision_scales))])
            weights[-1] = 0
            weights = weights / weights.sum()
            loss = losses.DeepSupervisionWrapper(loss, weights)
        return loss

    def set_deep_supervision_enabled(self, enabled: bool):
        self.network.decoder.deep_supervision = enabled

    def on_train_epoch_start(self):
        self.network.train()
        self.lr_scheduler.step(self.current_epoch)

    # -- synthetic batch (the reference's own benchmark harness) ---------------------------------------------
    def make_dummy_batch(self, seed=None):
        """nnUNetTrainerBenchmark_5epochs_noDataLoading.py:16-22."""
        g = torch.Generator(device='cpu')
        g.manual_seed(1234 + self.local_rank if seed is None else seed)
        patch_size = self.configuration_manager.patch_size
        data = torch.rand((self.batch_size, self.num_input_channels, *patch_size), generator=g)
        target = [torch.round(torch.rand((self.batch_size, 1, *[int(i * j) for i, j in zip(patch_size, k)]),
                                         generator=g) * max(self.label_manager.all_labels))
                  for k in self._get_deep_supervision_scales()]
        return {'data': data.to(self.device), 'target': [t.to(self.device) for t in target]}

    # -- the hot path ---------------------------------------------------------------------------------------
    def _forward_loss(self, data, target):
        output = self.network(data)
        return self.loss(output, target), output

    def _step_body(self, data, target):
        """zero_grad -> forward -> loss -> backward -> (gradient all-reduce fence) -> clip + SGD (:901-924)."""
        if self.reducer is not None:
            self.reducer.reset()   # a backward() that raised last step must not leave stale bucket state behind
        self.optimizer.zero_grad(set_to_none=True)
        l, _ = self._forward_loss(data, target)
        l.backward()
        if self.reducer is not None:
            self.reducer.wait()
        self.optimizer.step()  # clip_grad_norm_(12) + SGD fused, clip coefficient stays on the device
        return l.detach()

    # -- the step as ONE hipGraph launch --------------------------------------------------------------------------
    # The ~400 kernels of a step are enqueued by Python in 11-12 ms; the bf16 step needs 13 ms of device time and the
    # reference's per-step `loss.cpu()` (:925) keeps the host from running ahead, so the device idles ~1.5 ms per step
    # between launches (profiles/r02_bf16_step_per_launch.txt: span - sum of durations).  After `hip_graph_warmup` eager
    # steps the step body is captured once per input geometry (torch.cuda.graph = hipGraph on ROCm) and replayed:
    # identical kernels, arguments and order -> results bit-identical to the eager step (tests/test_gpu_graph.py).
    # What keeps that valid: inputs are copied into static buffers; the optimizer's scalars live in device memory
    # (mvd_sgd_nesterov_step_dev: PolyLR needs no re-capture); the packed weight copies are rewritten in place by the
    # captured repack (FlatParams.pack16_inplace); nothing in the body synchronises or depends on host-side data.
    def _graph_allowed(self):
        if not self.use_hip_graph:
            return False
        if self.reducer is not None and self.reducer.world > 1:
            # collectives inside a capture: RCCL supports it, but it is unverified here on more than one GPU
            return os.environ.get("MVD_HIPGRAPH_DDP", "0") == "1" and dist.get_backend() == "nccl"
        return True

    def _graph_key(self, data, target):
        tl = target if isinstance(target, (list, tuple)) else [target]
        return (tuple(data.shape), data.dtype, tuple((tuple(t.shape), t.dtype) for t in tl), isinstance(target, list),
                self.precision, self.network.training, self._graph_flags())

    def _label_mode(self):
        lm = self.label_manager
        return (lm.has_regions, tuple(lm.foreground_regions) if lm.has_regions else None, lm.ignore_label)

    def _graph_flags(self):
        return (bool(self.network.decoder.deep_supervision), self._label_mode())

    def _graph_side_outputs(self):
        """Device tensors the step body leaves on the trainer beside the loss (none here), collected after the capture."""
        return None

    def _restore_graph_side_outputs(self, side):
        """Called after every replay with what _graph_side_outputs() returned: a replay runs no Python, and an eager
        forward in between (validation_step) may have re-pointed the attributes at its own tensors."""

    def _graphed_step(self, data, target):
        key = self._graph_key(data, target)
        sg = self._step_graph
        if sg is None or sg['key'] != key:
            sg = self._step_graph = {'key': key, 'graph': None, 'warm': 0}
        # Invariant: every packed weight a replay reads is either rewritten by the replay itself (the captured repack, for
        # the NEXT replay) or refreshed before it.  load_state_dict / invalidate_packs since the last step leave stale
        # stamps -> repack first: before a replay, before the capture (no pack kernel may be captured by accident) and
        # before a warm-up step (one batched launch instead of a rewrite per layer).  An eager forward in between
        # (validation_step) that met a stale entry has packed it IN PLACE into the persistent buffer
        # (ops._pack16_rewrite), so a current stamp always means a current buffer.
        if ops.packs_stale(self.optimizer.fp):
            ops.repack_all(self.optimizer.fp)
        if sg['graph'] is None:
            if sg['warm'] < self.hip_graph_warmup:
                sg['warm'] += 1   # eager first: allocator steady state, the optimizer's first-step flag, pack caches
                return self._step_body(data, target)
            sg['data'] = data.clone()
            sg['target'] = [t.clone() for t in target] if isinstance(target, list) else target.clone()
            self.optimizer.use_device_hyper()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g):
                    sg['loss'] = self._step_body(sg['data'], sg['target'])
            except Exception as e:  # leave the eager path intact and say so (no silent slow path)
                self.use_hip_graph = False
                self._step_graph = None
                torch.cuda.synchronize()
                import warnings
                warnings.warn(f"hipGraph capture of the train step failed ({type(e).__name__}: {e}); running eagerly")
                return self._step_body(data, target)
            sg['graph'] = g
            sg['side'] = self._graph_side_outputs()
            captured_now = True    # (the capture ran the body's Python once: the optimizer's step counter already moved)
        else:
            captured_now = False
            if sg['data'].data_ptr() != data.data_ptr():
                sg['data'].copy_(data, non_blocking=True)
            if isinstance(target, list):
                for st, t in zip(sg['target'], target):
                    if st.data_ptr() != t.data_ptr():
                        st.copy_(t, non_blocking=True)
            elif sg['target'].data_ptr() != target.data_ptr():
                sg['target'].copy_(target, non_blocking=True)
        self.optimizer.sync_hyper()
        sg['graph'].replay()
        self._restore_graph_side_outputs(sg['side'])
        if not captured_now:
            self.optimizer.note_replayed_step()
        return sg['loss']

    # -- training feed (nnUNetTrainer.py:377-434 and :600-630, fed from HBM by dataloading.DeviceDataLoader3D) ----
    def configure_rotation_dummyDA_mirroring_and_inital_patch_size(self):
        """nnUNetTrainer.py:377-434 (ANISO_THRESHOLD = 3, configuration.py:7).  3-D plans, both branches: an isotropic
        patch rotates about every axis by +-30 degrees; an anisotropic one (max / patch[0] > 3) takes the dummy 2-D
        mode -- in-plane rotation by +-180 degrees, axis 0 of the initial patch kept -- which the device feed runs with
        its in-plane kernels.  2-D plans (:386-401): no dummy mode, rotation about x by +-15 degrees when
        max / min of the patch exceeds 1.5 and by +-180 degrees otherwise, mirroring over both axes."""
        patch_size = self.configuration_manager.patch_size
        dim = len(patch_size)
        if dim not in (2, 3):
            raise NotImplementedError("configure_rotation_dummyDA_mirroring_and_inital_patch_size: 2-D and 3-D plans only")
        if dim == 2:
            do_dummy_2d_data_aug = False
            deg = 15. if max(patch_size) / min(patch_size) > 1.5 else 180.
            rotation_for_DA = {'x': (-deg / 360 * 2. * np.pi, deg / 360 * 2. * np.pi), 'y': (0, 0), 'z': (0, 0)}
            mirror_axes = (0, 1)
        else:
            do_dummy_2d_data_aug = (max(patch_size) / patch_size[0]) > ANISO_THRESHOLD
            if do_dummy_2d_data_aug:
                rotation_for_DA = {'x': (-180. / 360 * 2. * np.pi, 180. / 360 * 2. * np.pi), 'y': (0, 0), 'z': (0, 0)}
            else:
                rotation_for_DA = {ax: (-30. / 360 * 2. * np.pi, 30. / 360 * 2. * np.pi) for ax in ('x', 'y', 'z')}
            mirror_axes = (0, 1, 2)
        # the reference sizes the initial patch with (0.85, 1.25), not the (0.7, 1.4) the transform draws from
        initial_patch_size = get_patch_size(patch_size[-dim:], *rotation_for_DA.values(), (0.85, 1.25))
        if do_dummy_2d_data_aug:
            initial_patch_size[0] = patch_size[0]
        self.inference_allowed_mirroring_axes = mirror_axes
        return rotation_for_DA, do_dummy_2d_data_aug, initial_patch_size, mirror_axes

    def get_device_dataloader(self, dataset_tr, device=None, intensity_augmentation=False, cascade_augmentation=True):
        """The training loader of get_dataloaders (:600-630) with its transforms' geometric part on the device: initial
        patch, SpatialTransform (rotation, scaling 0.7-1.4), mirroring, RemoveLabel and the deep-supervision targets.
        intensity_augmentation=True adds the intensity transforms (:719-736) and, where the plans set
        use_mask_for_norm, MaskTransform: the reference's whole training recipe.  A cascaded trainer's loader runs in
        cascade mode (dataset cases carry the previous stage's segmentation as seg channel 1): the one-hot move and, unless
        cascade_augmentation=False, the binary operators and the component removal (:740-755)."""
        self._check_cascade()
        rotation_for_DA, do_dummy_2d_data_aug, initial_patch_size, mirror_axes = \
            self.configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        if len(self.configuration_manager.patch_size) == 2:
            # nnUNetDataLoader2D (:612-617): slices of the resident cases, geometric transforms on the device
            if intensity_augmentation:
                raise NotImplementedError("the intensity stage of the device feed is not built for the 2d configuration")
            return DeviceDataLoader2D(dataset_tr, self.batch_size, [int(i) for i in initial_patch_size],
                                      self.configuration_manager.patch_size, self.label_manager,
                                      oversample_foreground_percent=self.oversample_foreground_percent,
                                      mirror_axes=mirror_axes, deep_supervision_scales=self._get_deep_supervision_scales(),
                                      device=self.device if device is None else device, rotation_for_DA=rotation_for_DA,
                                      scale_range=(0.7, 1.4))
        use_mask_for_norm = getattr(self.configuration_manager, 'use_mask_for_norm', None)
        mask_channels = use_mask_for_norm if intensity_augmentation and use_mask_for_norm else None
        return DeviceDataLoader3D(dataset_tr, self.batch_size, [int(i) for i in initial_patch_size],
                                  self.configuration_manager.patch_size, self.label_manager,
                                  oversample_foreground_percent=self.oversample_foreground_percent,
                                  mirror_axes=mirror_axes, deep_supervision_scales=self._get_deep_supervision_scales(),
                                  device=self.device if device is None else device, rotation_for_DA=rotation_for_DA,
                                  scale_range=(0.7, 1.4), do_dummy_2d_data_aug=do_dummy_2d_data_aug,
                                  intensity_augmentation=intensity_augmentation, mask_channels=mask_channels,
                                  cascade_labels=self.label_manager.foreground_labels if self.is_cascaded else None,
                                  cascade_augmentation=cascade_augmentation and self.is_cascaded)

    def get_device_validation_dataloader(self, dataset_val, device=None):
        """The validation loader of get_dataloaders with get_validation_transforms (:771-802): final patch straight from
        the case, no spatial, intensity or mirror stage, RemoveLabel, for a cascaded trainer the one-hot move alone
        (:783-784), and the deep-supervision targets."""
        self._check_cascade()
        if len(self.configuration_manager.patch_size) == 2:
            return DeviceDataLoader2D(dataset_val, self.batch_size, self.configuration_manager.patch_size,
                                      self.configuration_manager.patch_size, self.label_manager,
                                      oversample_foreground_percent=self.oversample_foreground_percent,
                                      deep_supervision_scales=self._get_deep_supervision_scales(),
                                      device=self.device if device is None else device)
        return DeviceDataLoader3D(dataset_val, self.batch_size, self.configuration_manager.patch_size,
                                  self.configuration_manager.patch_size, self.label_manager,
                                  oversample_foreground_percent=self.oversample_foreground_percent,
                                  deep_supervision_scales=self._get_deep_supervision_scales(),
                                  device=self.device if device is None else device,
                                  cascade_labels=self.label_manager.foreground_labels if self.is_cascaded else None,
                                  cascade_augmentation=False)

    def train_step(self, batch: dict, return_device_loss: bool = False) -> dict:
        data, target = batch['data'], batch['target']
        data = data.to(self.device, non_blocking=True)
        if isinstance(target, list):
            target = [i.to(self.device, non_blocking=True) for i in target]
        else:
            target = target.to(self.device, non_blocking=True)
        l = self._graphed_step(data, target) if self._graph_allowed() else self._step_body(data, target)
        if return_device_loss:
            # the graph's loss is ONE static tensor that every replay overwrites: hand out a copy, as the eager step does
            sg = self._step_graph
            return {'loss': l.clone() if sg is not None and l is sg.get('loss') else l}
        return {'loss': l.cpu().numpy()}  # the reference syncs here every step (:925)

    def validation_step(self, batch: dict) -> dict:
        data, target = batch['data'], batch['target']
        data = data.to(self.device, non_blocking=True)
        target = [i.to(self.device, non_blocking=True) for i in target] if isinstance(target, list) \
            else target.to(self.device, non_blocking=True)
        # on_validation_epoch_start (:939-940) puts the network in eval(); a caller that validates between train steps gets
        # the same here, and its mode back afterwards.  Only BatchNorm reads the flag: running statistics, left untouched.
        was_training = self.network.training
        self.network.eval()
        try:
            with torch.no_grad():
                l, output = self._forward_loss(data, target)
        finally:
            self.network.train(was_training)
        with torch.no_grad():
            if self.enable_deep_supervision:
                output, target = output[0], target[0]
            lm = self.label_manager
            if lm.has_regions:     # (:969-970, :985-989) sigmoid heads, every head is foreground: no [1:]
                counts = ops.sigmoid_counts(output, target, lm.foreground_regions, lm.ignore_label).cpu().numpy()
            elif lm.has_ignore_label:   # (:980-984)
                counts = ops.argmax_counts_masked(output, target, lm.ignore_label).cpu().numpy()[1:]
            else:
                counts = ops.argmax_counts(output, target).cpu().numpy()[1:]  # [1:] removes background (:996-1002)
        tp_hard, fp_hard, fn_hard = counts[:, 0], counts[:, 1], counts[:, 2]
        return {'loss': l.detach().cpu().numpy(), 'tp_hard': tp_hard, 'fp_hard': fp_hard, 'fn_hard': fn_hard}

    # -- final validation (nnUNetTrainer.py:1135-1260) for in-memory cases, everything on the device ---------------
    def perform_actual_validation(self, cases, save_probabilities: bool = False, pp_fns=None, pp_fn_kwargs=None,
                                  tile_step_size: float = 0.5, use_gaussian: bool = True, use_mirroring: bool = True,
                                  return_segmentations: bool = False, surface_metrics: bool = False,
                                  surface_connectivity: int = 1, return_next_stage: bool = False):
        """`cases`: dicts {'data': preprocessed image [C, d, h, w], 'properties': the case's properties dict
        (shape_before_cropping, bbox_used_for_cropping, shape_after_cropping_and_before_resampling, spacing), 'seg':
        ground truth in the original space (uint8 / int16, [D, H, W] or [1, D, H, W])}.  Per case: sliding-window
        prediction (tile step 0.5, Gaussian, mirroring: the reference's settings :1140-1142) -> segmentation export
        (export.py) -> optional postprocessing.apply_postprocessing(pp_fns, pp_fn_kwargs) -> confusion counts, with one
        host synchronisation per case (the counts).  Returns compute_metrics_on_folder's {'metric_per_case', 'mean',
        'foreground_mean'}; with return_segmentations also the list of device segmentations (and with
        save_probabilities the list of probability volumes).  surface_metrics adds 'HD', 'HD95' and 'ASSD' (evaluation.
        compute_surface_metrics, spacing = properties['spacing'], footprint surface_connectivity) to every per-case,
        per-label dict, and with them to the means.  Deep supervision is off for the duration and restored.
        A cascaded trainer (:1175-1177) needs case['seg_prev'], the previous stage's segmentation in this stage's
        preprocessed space [d, h, w]: it is one-hot encoded on the device and stacked behind the image.  For a
        configuration with next_stage_names (:1207-1238) a case may carry 'next_stage_shapes' = {stage name: preprocessed
        shape of the case in that stage}; with return_next_stage the logits are resampled to each
        (export.resample_logits_for_next_stage) and the result gains a last element, one {stage name: uint8 [shape]} dict
        per case -- a stage without a shape is skipped, as the reference skips a case whose preprocessed file is missing.
        Files and the worker pool are out of scope."""
        from . import evaluation, export, postprocessing
        from .inference import SlidingWindowPredictor
        if not hasattr(self, 'inference_allowed_mirroring_axes'):
            self.configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        ds_holder = self.network.decoder if hasattr(self.network, 'decoder') else self.network
        ds_attr = 'deep_supervision' if hasattr(self.network, 'decoder') else 'do_ds'
        ds_before = getattr(ds_holder, ds_attr)
        was_training = self.network.training
        self.set_deep_supervision_enabled(False)
        self.network.eval()
        labels = self.label_manager.foreground_regions if self.label_manager.has_regions \
            else self.label_manager.foreground_labels
        results, segs, probs, next_stage = [], [], [], []
        self._check_cascade()
        next_stages = getattr(self.configuration_manager, 'next_stage_names', None)
        try:
            predictor = SlidingWindowPredictor(self.network, self.configuration_manager.patch_size,
                                               self.label_manager.num_segmentation_heads, tile_step_size=tile_step_size,
                                               use_gaussian=use_gaussian, use_mirroring=use_mirroring,
                                               allowed_mirroring_axes=self.inference_allowed_mirroring_axes,
                                               device=self.device)
            for case in cases:
                data = case['data']
                if self.is_cascaded:
                    data = self._stack_previous_stage(data, case.get('seg_prev'))
                prediction = predictor.predict_sliding_window_return_logits(data)
                if return_next_stage:
                    shapes = case.get('next_stage_shapes') or {}
                    next_stage.append({n: export.resample_logits_for_next_stage(
                        prediction, shapes[n], self.configuration_manager, self.label_manager)
                        for n in (next_stages or []) if n in shapes})
                out = export.convert_predicted_logits_to_segmentation_with_correct_shape(
                    prediction, self.plans_manager, self.configuration_manager, self.label_manager, case['properties'],
                    return_probabilities=save_probabilities)
                seg = out[0] if save_probabilities else out
                del prediction
                if pp_fns:
                    seg = postprocessing.apply_postprocessing(seg, pp_fns, pp_fn_kwargs)
                ref = case['seg']
                ref = torch.from_numpy(np.ascontiguousarray(ref)) if isinstance(ref, np.ndarray) else ref
                ref = ref.to(self.device, non_blocking=True)
                if ref.dim() == 4:
                    ref = ref[0]
                if tuple(ref.shape) != tuple(seg.shape):
                    raise RuntimeError(f"ground truth {tuple(ref.shape)} and exported segmentation {tuple(seg.shape)} "
                                       f"differ in shape")
                results.append(evaluation.compute_metrics(ref, seg, labels, self.label_manager.ignore_label))
                if surface_metrics:
                    surf = evaluation.compute_surface_metrics(ref, seg, labels, case['properties']['spacing'],
                                                              surface_connectivity, self.label_manager.ignore_label)
                    for key, m in surf.items():
                        results[-1]['metrics'][key].update(m)
                if return_segmentations:
                    segs.append(seg)
                    if save_probabilities:
                        probs.append(out[1])
        finally:
            setattr(ds_holder, ds_attr, ds_before)
            self.network.train(was_training)
        if not results:
            raise ValueError("perform_actual_validation: no cases")
        metrics = evaluation.aggregate_metrics(results, labels)
        ret = (metrics,)
        if return_segmentations:
            ret = (metrics, segs, probs) if save_probabilities else (metrics, segs)
        if return_next_stage:
            ret = ret + (next_stage,)
        return ret if len(ret) > 1 else metrics

    def _stack_previous_stage(self, data, seg_prev):
        """:1175-1177: data [C, d, h, w] with convert_labelmap_to_one_hot(seg_prev, foreground_labels) behind it, built on
        the device by the feed's one-hot kernel."""
        from .dataloading import cascade_onehot
        if seg_prev is None:
            raise ValueError("perform_actual_validation: a cascaded trainer (previous_stage_name "
                             f"'{self.configuration_manager.previous_stage_name}') needs case['seg_prev'], the previous "
                             "stage's segmentation in this stage's preprocessed space")
        data = torch.as_tensor(np.ascontiguousarray(data) if isinstance(data, np.ndarray) else data,
                               dtype=torch.float32).to(self.device)
        prev = torch.as_tensor(np.ascontiguousarray(seg_prev) if isinstance(seg_prev, np.ndarray) else seg_prev)
        prev = prev.to(self.device).to(torch.float32).contiguous()
        if prev.dim() == 4 and prev.shape[0] == 1:
            prev = prev[0]
        if tuple(prev.shape) != tuple(data.shape[1:]):
            raise ValueError(f"perform_actual_validation: seg_prev {tuple(prev.shape)} and the image {tuple(data.shape[1:])} "
                             "differ in shape")
        labels = self.label_manager.foreground_labels
        out = torch.empty((data.shape[0] + len(labels), *data.shape[1:]), dtype=torch.float32, device=self.device)
        out[:data.shape[0]] = data
        cascade_onehot(prev, out[data.shape[0]:], labels)
        return out

    @staticmethod
    def dice_from_counts(tp, fp, fn):
        """on_validation_epoch_end :1033-1034."""
        with np.errstate(divide='ignore', invalid='ignore'):
            per_class = [2 * i / (2 * i + j + k) for i, j, k in zip(tp, fp, fn)]
        return per_class, float(np.nanmean(per_class))


class nnUNetTrainerMI355Benchmark_noDataLoading(nnUNetTrainerMI355):
    """variants/benchmarking/nnUNetTrainerBenchmark_5epochs_noDataLoading.py:8-51: constant synthetic batch."""

    def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=torch.device('cuda')):
        super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device)
        self.num_epochs = 5
        self.dummy_batch = None

    def initialize(self):
        super().initialize()
        self.dummy_batch = self.make_dummy_batch()


class nnUNetTrainerBNMI355(nnUNetTrainerMI355):
    """variants/network_architecture/nnUNetTrainerBN.py:10-42: the same trainer with BatchNorm3d in place of
    InstanceNorm3d -- only the static network builder differs.  The running statistics are module buffers (not in
    FlatParams): the training kernels update them on the device, so the eager and the graphed step move them alike, and
    eval() (validation_step, perform_actual_validation, the sliding-window predictor) reads them without writing.  Under
    data parallelism every rank keeps its own buffers and rank 0's are the ones to save, which is the checkpoint torch
    DDP (broadcast_buffers=True) writes."""

    @staticmethod
    def build_network_architecture(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                   enable_deep_supervision: bool = True) -> nn.Module:
        return get_network_from_plans(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                      deep_supervision=enable_deep_supervision, norm_op=nn.BatchNorm3d,
                                      norm_op_kwargs={'eps': 1e-5, 'affine': True})


# ------------------------------------------------------------------------------------------------ optimizer / schedule variants
class nnUNetTrainerAdamMI355(nnUNetTrainerMI355):
    """variants/optimizer/nnUNetTrainerAdam.py:8-17: AdamW(lr, weight_decay, amsgrad=True) with PolyLR.  Like the
    reference's class it overrides configure_optimizers alone; clip_grad_norm_(12) belongs to train_step (:918) and
    stays fused into the update (optim.FusedAdam)."""

    def configure_optimizers(self):
        optimizer = FusedAdam(self._flat_params(), lr=self.initial_lr, weight_decay=self.weight_decay, amsgrad=True,
                              decoupled_weight_decay=True, max_grad_norm=12)
        lr_scheduler = PolyLRScheduler(optimizer, self.initial_lr, self.num_epochs)
        return optimizer, lr_scheduler


class nnUNetTrainerVanillaAdamMI355(nnUNetTrainerMI355):
    """nnUNetTrainerAdam.py:20-28: Adam(lr, weight_decay) (L2 weight decay, no amsgrad) with PolyLR."""

    def configure_optimizers(self):
        optimizer = FusedAdam(self._flat_params(), lr=self.initial_lr, weight_decay=self.weight_decay, max_grad_norm=12)
        lr_scheduler = PolyLRScheduler(optimizer, self.initial_lr, self.num_epochs)
        return optimizer, lr_scheduler


class nnUNetTrainerVanillaAdam1en3MI355(nnUNetTrainerVanillaAdamMI355):
    def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=torch.device('cuda'),
                 specified_cfg=''):
        super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device, specified_cfg)
        self.initial_lr = 1e-3   # nnUNetTrainerAdam.py:35


class nnUNetTrainerVanillaAdam3en4MI355(nnUNetTrainerVanillaAdamMI355):
    def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=torch.device('cuda'),
                 specified_cfg=''):
        super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device, specified_cfg)
        self.initial_lr = 3e-4   # :43


class nnUNetTrainerAdam1en3MI355(nnUNetTrainerAdamMI355):
    def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=torch.device('cuda'),
                 specified_cfg=''):
        super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device, specified_cfg)
        self.initial_lr = 1e-3   # :50


class nnUNetTrainerAdam3en4MI355(nnUNetTrainerAdamMI355):
    def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=torch.device('cuda'),
                 specified_cfg=''):
        super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device, specified_cfg)
        self.initial_lr = 3e-4   # :58


class nnUNetTrainerCosAnnealMI355(nnUNetTrainerMI355):
    """variants/lr_schedule/nnUNetTrainerCosAnneal.py:7-12: the base trainer's SGD with CosineAnnealingLR(T_max=num_epochs)."""

    def configure_optimizers(self):
        optimizer = FusedSGDNesterov(self._flat_params(), self.initial_lr, weight_decay=self.weight_decay, momentum=0.99,
                                     nesterov=True, max_grad_norm=12)
        lr_scheduler = CosineAnnealingLR(optimizer, T_max=self.num_epochs)
        return optimizer, lr_scheduler


# ------------------------------------------------------------------------------------------------ loss variants
def _variant_checks(tr, what, regions_ok=False):
    """What every loss variant refuses before it builds anything: cascades (as the base trainer), more heads than the loss
    kernels hold, and -- where the reference's class asserts it -- regions."""
    if getattr(tr.configuration_manager, 'previous_stage_name', None) is not None:
        raise NotImplementedError(f"{what}: cascade configurations (previous_stage_name) are built for the base trainer's "
                                  "loss only, not for the loss variants")
    if not regions_ok:
        assert not tr.label_manager.has_regions, 'regions not supported by this trainer'
    if tr.label_manager.num_segmentation_heads > ops.REGION_KMAX:
        raise NotImplementedError(f"{what}: {tr.label_manager.num_segmentation_heads} segmentation heads: the fused loss "
                                  f"kernels hold at most {ops.REGION_KMAX}")


def _wrap_every_level(tr, loss):
    """variants/loss/*.py: weights 1 / 2^i over ALL deep-supervision levels, normalised -- the base trainer's
    `weights[-1] = 0` is absent from these classes, so the coarsest level contributes too."""
    if not tr.enable_deep_supervision:
        return loss
    weights = np.array([1 / (2 ** i) for i in range(len(tr._get_deep_supervision_scales()))])
    return losses.DeepSupervisionWrapper(loss, weights / weights.sum())


def _check_topk_levels(tr, what, k_percent):
    """k = int(voxels of the level * k / 100) must be >= 1 on every level the loss sees (the reference returns NaN there)."""
    cm = tr.configuration_manager
    scales = tr._get_deep_supervision_scales() or [[1] * len(cm.patch_size)]
    batch = 1 if tr.is_ddp else int(cm.batch_size)   # (a rank of a data-parallel run holds at least one sample)
    for s in scales:
        n = batch * int(np.prod([int(i * j) for i, j in zip(cm.patch_size, s)]))
        if ops.topk_count(n, k_percent) < 1:
            raise NotImplementedError(f"{what}: a deep-supervision level of {n} voxels gives k = int({n} * {k_percent} / 100) "
                                      f"= 0, where the reference's loss is NaN; use a larger patch or fewer levels")


class nnUNetTrainerDiceLossMI355(nnUNetTrainerMI355):
    """variants/loss/nnUNetTrainerDiceLoss.py:11-27: soft Dice alone, do_bg = has_regions, sigmoid heads for regions
    (DC_and_BCE_loss with weight_ce = 0: the same Dice over the same heads).  With an ignore label the reference's loss
    has no mask (the target then carries one plane more than the network has heads) and cannot run: refused."""

    def _build_loss(self):
        _variant_checks(self, "nnUNetTrainerDiceLossMI355", regions_ok=True)
        if self.label_manager.has_ignore_label:
            raise NotImplementedError("nnUNetTrainerDiceLossMI355: the reference's Dice-only loss has no mask for the ignore "
                                      "label and cannot run on such plans")
        kw = {'batch_dice': self.configuration_manager.batch_dice, 'do_bg': self.label_manager.has_regions, 'smooth': 1e-5,
              'ddp': self.is_ddp}
        if self.label_manager.has_regions:
            loss = losses.DC_and_BCE_loss({}, kw, weight_ce=0, weight_dice=1, use_ignore_label=False,
                                          dice_class=losses.MemoryEfficientSoftDiceLoss,
                                          regions=self.label_manager.foreground_regions, ignore_label=None)
        else:
            loss = losses.MemoryEfficientSoftDiceLoss(**kw)
        return _wrap_every_level(self, loss)


class nnUNetTrainerDiceCELoss_noSmoothMI355(nnUNetTrainerMI355):
    """nnUNetTrainerDiceLoss.py:30-55: the base trainer's loss with smooth = 0 (the 1e-8 clip of the denominator stays)."""

    def _build_loss(self):
        _variant_checks(self, "nnUNetTrainerDiceCELoss_noSmoothMI355", regions_ok=True)
        if self.label_manager.has_regions:
            loss = losses.DC_and_BCE_loss({}, {'batch_dice': self.configuration_manager.batch_dice, 'do_bg': True,
                                               'smooth': 0, 'ddp': self.is_ddp},
                                          use_ignore_label=self.label_manager.ignore_label is not None,
                                          dice_class=losses.MemoryEfficientSoftDiceLoss,
                                          regions=self.label_manager.foreground_regions,
                                          ignore_label=self.label_manager.ignore_label)
        else:
            loss = losses.DC_and_CE_loss({'batch_dice': self.configuration_manager.batch_dice, 'smooth': 0, 'do_bg': False,
                                          'ddp': self.is_ddp}, {}, weight_ce=1, weight_dice=1,
                                         ignore_label=self.label_manager.ignore_label,
                                         dice_class=losses.MemoryEfficientSoftDiceLoss)
        return _wrap_every_level(self, loss)


class nnUNetTrainerCELossMI355(nnUNetTrainerMI355):
    """variants/loss/nnUNetTrainerCELoss.py: cross entropy alone, the ignore label as its ignore_index."""

    def _build_loss(self):
        _variant_checks(self, "nnUNetTrainerCELossMI355")
        lm = self.label_manager
        loss = losses.RobustCrossEntropyLoss(weight=None, ignore_index=lm.ignore_label if lm.has_ignore_label else -100)
        return _wrap_every_level(self, loss)


class nnUNetTrainerTopk10LossMI355(nnUNetTrainerMI355):
    """variants/loss/nnUNetTrainerTopkLoss.py:8-24: the mean of the largest 10 % of the per-voxel cross entropy."""

    def _build_loss(self):
        _variant_checks(self, "nnUNetTrainerTopk10LossMI355")
        _check_topk_levels(self, "nnUNetTrainerTopk10LossMI355", 10)
        lm = self.label_manager
        loss = losses.TopKLoss(ignore_index=lm.ignore_label if lm.has_ignore_label else -100, k=10)
        return _wrap_every_level(self, loss)


class nnUNetTrainerTopk10LossLS01MI355(nnUNetTrainerMI355):
    """nnUNetTrainerTopkLoss.py:27-43: the same with label_smoothing = 0.1."""

    def _build_loss(self):
        _variant_checks(self, "nnUNetTrainerTopk10LossLS01MI355")
        _check_topk_levels(self, "nnUNetTrainerTopk10LossLS01MI355", 10)
        lm = self.label_manager
        loss = losses.TopKLoss(ignore_index=lm.ignore_label if lm.has_ignore_label else -100, k=10, label_smoothing=0.1)
        return _wrap_every_level(self, loss)


class nnUNetTrainerDiceTopK10LossMI355(nnUNetTrainerMI355):
    """nnUNetTrainerTopkLoss.py:46-66: soft Dice (no background, smooth 1e-5) + top-10 % cross entropy."""

    def _build_loss(self):
        _variant_checks(self, "nnUNetTrainerDiceTopK10LossMI355")
        _check_topk_levels(self, "nnUNetTrainerDiceTopK10LossMI355", 10)
        loss = losses.DC_and_topk_loss({'batch_dice': self.configuration_manager.batch_dice, 'smooth': 1e-5, 'do_bg': False,
                                        'ddp': self.is_ddp}, {'k': 10, 'label_smoothing': 0.0}, weight_ce=1, weight_dice=1,
                                       ignore_label=self.label_manager.ignore_label)
        return _wrap_every_level(self, loss)


# ------------------------------------------------------------------------------------------------ data augmentation variants
class nnUNetTrainerDA5MI355(nnUNetTrainerMI355):
    """variants/data_augmentation/nnUNetTrainerDA5.py: the heavier augmentation recipe, run by the device feed.
    3-D plans without the dummy 2-D mode and without a cascade; everything else is refused with a message."""

    def configure_rotation_dummyDA_mirroring_and_inital_patch_size(self):
        """nnUNetTrainerDA5.py:36-91: the base trainer's rotations, mirroring and dummy-2-D rule; the initial patch is sized
        with the scale range (0.7, 1.43)."""
        rotation_for_DA, do_dummy_2d_data_aug, _, mirror_axes = \
            super().configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        patch_size = self.configuration_manager.patch_size
        dim = len(patch_size)
        initial_patch_size = get_patch_size(patch_size[-dim:], *rotation_for_DA.values(), (0.7, 1.43))
        if do_dummy_2d_data_aug:
            initial_patch_size[0] = patch_size[0]
        return rotation_for_DA, do_dummy_2d_data_aug, initial_patch_size, mirror_axes

    def get_device_dataloader(self, dataset_tr, device=None, intensity_augmentation=True, cascade_augmentation=True,
                              da5_probabilities=None):
        """The training loader with da5=True (nnUNetTrainerDA5.get_training_transforms:94-305): SpatialTransform with
        p_rot_per_sample 0.4, p_rot_per_axis 0.5, p_scale_per_sample 0.2, scale (0.7, 1.43) independently per axis, then
        the DA5 chain.  The intensity stage is implied."""
        if len(self.configuration_manager.patch_size) != 3:
            raise NotImplementedError("nnUNetTrainerDA5MI355: DA5 is built for 3-D plans only")
        if self.is_cascaded:
            raise NotImplementedError("nnUNetTrainerDA5MI355: DA5 with a cascade is not built")
        rotation_for_DA, do_dummy_2d_data_aug, initial_patch_size, mirror_axes = \
            self.configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        if do_dummy_2d_data_aug:
            raise NotImplementedError("nnUNetTrainerDA5MI355: DA5 for an anisotropic plan (do_dummy_2d_data_aug, the "
                                      "in-plane form of the recipe) is not built")
        use_mask_for_norm = getattr(self.configuration_manager, 'use_mask_for_norm', None)
        return DeviceDataLoader3D(dataset_tr, self.batch_size, [int(i) for i in initial_patch_size],
                                  self.configuration_manager.patch_size, self.label_manager,
                                  oversample_foreground_percent=self.oversample_foreground_percent,
                                  mirror_axes=mirror_axes, deep_supervision_scales=self._get_deep_supervision_scales(),
                                  device=self.device if device is None else device, rotation_for_DA=rotation_for_DA,
                                  scale_range=(0.7, 1.43), p_rot_per_sample=0.4, p_rot_per_axis=0.5,
                                  p_scale_per_sample=0.2, mask_channels=use_mask_for_norm if use_mask_for_norm else None,
                                  da5=True, da5_probabilities=da5_probabilities)


class nnUNetTrainerDA5_10epochsMI355(nnUNetTrainerDA5MI355):
    """nnUNetTrainerDA5.py: nnUNetTrainerDA5_10epochs."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.num_epochs = 10


class nnUNetTrainerNoMirroringMI355(nnUNetTrainerMI355):
    """variants/data_augmentation/nnUNetTrainerNoMirroring.py:4-10: no mirroring in training, none at inference."""

    def configure_rotation_dummyDA_mirroring_and_inital_patch_size(self):
        rotation_for_DA, do_dummy_2d_data_aug, initial_patch_size, _ = \
            super().configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        self.inference_allowed_mirroring_axes = None
        return rotation_for_DA, do_dummy_2d_data_aug, initial_patch_size, None


class nnUNetTrainerNoDAMI355(nnUNetTrainerMI355):
    """variants/data_augmentation/nnUNetTrainerNoDA.py: the training loader runs the validation transforms -- final patch
    straight from the case, no spatial, intensity or mirror stage -- and inference does not mirror."""

    def configure_rotation_dummyDA_mirroring_and_inital_patch_size(self):
        rotation_for_DA, do_dummy_2d_data_aug, _, _ = super().configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        self.inference_allowed_mirroring_axes = None
        return rotation_for_DA, do_dummy_2d_data_aug, self.configuration_manager.patch_size, None

    def get_device_dataloader(self, dataset_tr, device=None, intensity_augmentation=False, cascade_augmentation=True):
        self.configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        return self.get_device_validation_dataloader(dataset_tr, device=device)


# ------------------------------------------------------------------------------------------------ persistence topological loss
class nnUNetTrainerTopoLossMI355(nnUNetTrainerMI355):
    """The base trainer's loss plus the reference's persistence topological loss (training/loss/Topo_Loss.py:16-85) on the
    full-resolution output of a 2d plan with plain labels:

        l = L(out, t) + topo_lambda * l_topo(softmax(out[0]), betti_topo_label(t[0]), topo_classes)

    topo_lambda = 1 is the fork's lambda3 (MVDTrainer.py:134); topo_classes defaults to every foreground class; the Betti
    numbers of the label map are counted per step on the device (losses.betti_topo_label).  The loss, the layers and the
    diagrams are pinned to the reference's own code; THIS COMPOSITION IS NOT: the fork's step is broken at exactly this line
    (MVDTrainer.py:920 uses `self.topo_loss`, which is defined nowhere), so where and with which weight the term enters a
    step is this project's choice.  The y_raw (squared-difference) term of TopoLoss is left out of the step: the reference
    defines it for fine-tuning against a frozen first network; losses.TopoLoss itself keeps accepting it.
    The step runs eagerly: the pairing of the diagrams is a host sweep between two copies, which a captured graph cannot
    hold.  Refused with a message: 3-D plans, regions, an ignore label, cascades, bf16, and the graphed step."""

    def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=torch.device('cuda'),
                 specified_cfg=''):
        super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device, specified_cfg)
        what = type(self).__name__
        if len(self.configuration_manager.patch_size) != 2:
            raise NotImplementedError(f"{what} on 3-D plans: the reference's persistence layer (LevelSetLayer2D) is the "
                                      "Freudenthal triangulation of a 2-D image; 3-D cubical persistence is not built")
        if self.label_manager.has_regions:
            raise NotImplementedError(f"{what} with regions: the topological loss reads softmax probabilities of plain labels")
        if self.label_manager.has_ignore_label:
            raise NotImplementedError(f"{what} with an ignore label: the Betti numbers of a partly unlabelled map are undefined")
        if self.is_cascaded:
            raise NotImplementedError(f"{what}: cascade configurations (previous_stage_name) are 3-D; nnU-Net plans no 2-D "
                                      "cascade")
        self.use_hip_graph = False
        self.topo_lambda = 1
        self.topo_classes = None     # None: every foreground class
        self.topo_max_k = 20
        self.topo_loss = None
        self.last_topo = None        # the (detached, device) topological term of the last forward

    def _check_precision(self):
        if self.precision != 'fp32':
            raise NotImplementedError(f"{type(self).__name__} in {self.precision}: the bar lengths are differences of "
                                      "probabilities and the pairing compares them exactly; only fp32 is built")

    def initialize(self):
        self._check_precision()
        super().initialize()

    def _build_loss(self):
        self._check_precision()
        h, w = self.configuration_manager.patch_size
        self.topo_loss = losses.TopoLoss((int(w), int(h)), topo_weight=1, sqdiff_weight=0, max_k=self.topo_max_k)
        return super()._build_loss()

    def _graph_allowed(self):
        if self.use_hip_graph:
            raise RuntimeError(f"{type(self).__name__}: use_hip_graph = True, but the step cannot be captured: the persistence "
                               "pairing runs on the host between a D2H and an H2D copy.  Leave use_hip_graph = False")
        return False

    def _topo_term(self, output, target):
        top = output[0] if isinstance(output, (list, tuple)) else output
        t = target[0] if isinstance(target, (list, tuple)) else target
        C = top.shape[1]
        classes = list(range(1, C)) if self.topo_classes is None else [int(c) for c in self.topo_classes]
        if not classes or min(classes) < 1 or max(classes) >= C:
            raise ValueError(f"topo_classes {classes}: foreground classes 1..{C - 1}")
        y_pred = torch.cat([ops.SoftmaxSelectFn.apply(top, c) for c in range(C)], 1)
        with torch.no_grad():
            # row i of the label belongs to class i + 1, as TopoLoss pairs `idx` with channel idx + 1
            label = losses.betti_topo_label(t, C)[:, 1:]
        return self.topo_loss(y_pred, None, label, idx=[c - 1 for c in classes])

    def _forward_loss(self, data, target):
        output = self.network(data)
        l = self.loss(output, target)
        if self.topo_lambda:
            lt = self._topo_term(output, target)
            self.last_topo = lt.detach()
            l = l + self.topo_lambda * lt
        return l, output


# ------------------------------------------------------------------------------------------------ MVD dual branch
class ContrastiveTrainerMI355(nnUNetTrainerMI355):
    """Dual-branch mutual-distillation step (MVDTrainer.py:879-925):
    l = L(out1,t) + L(out2,t) + lambda3 * L_topo(out1[0][:,v], onehot(t)[:,v]) + lambda1 * L_KL.
    L_topo is soft-clDice on the softmax channel (topo_term = 'cldice', the default) or the reference's own term
    (topo_term = 'cubical'): losses.CubicalWassersteinLoss(topo_feat_d, topo_q) on the raw logit channel; that mode has a
    host sweep in the forward and runs eagerly only."""

    def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=torch.device('cuda'),
                 specified_cfg=''):
        super().__init__(plans, configuration, fold, dataset_json, unpack_dataset, device, specified_cfg)
        if len(self.configuration_manager.patch_size) != 3:
            raise NotImplementedError("ContrastiveTrainerMI355 on 2-D plans: the soft skeleton and the connected-component "
                                      "count of its topology term are 3-D kernels")
        if self.label_manager.has_regions or self.label_manager.has_ignore_label:
            raise NotImplementedError("ContrastiveTrainerMI355 with regions or an ignore label: its vessel-channel terms "
                                      "(softmax channel select, KL, soft-clDice) are defined for softmax heads only")
        self.lambda1, self.lambda2, self.lambda3 = 0.5, 0.1, 1  # MVDTrainer.py:132-134
        self.vessel_channel = 2                                 # :897-898, :907-908
        self.use_topo, self.skel_iter, self.feat_kl, self.kl_T = True, 3, True, 1
        self.topo_cc = True          # with use_topo: the integer connected-component count beside the soft-clDice term
        self.last_topology = None
        # 'cldice': the soft-clDice stand-in; 'cubical': the reference's own term, the Wasserstein distance between the 3-D
        # cubical diagrams of dimension topo_feat_d of the vessel logits and of the vessel mask (MVDTrainer.py:94-97, 907-925)
        self.topo_term, self.topo_feat_d, self.topo_q = 'cldice', 2, 2
        self.last_cubical = None     # the (detached, device) cubical term of the last forward

    @staticmethod
    def build_network_architecture(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                   enable_deep_supervision: bool = True) -> nn.Module:
        _refuse_residual_plans(configuration_manager, "ContrastiveTrainerMI355 (dual-branch)")
        b1 = get_network_from_plans(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                    enable_deep_supervision)
        b2 = get_network_from_plans(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                    enable_deep_supervision)
        return MVDDualBranchNet(b1, b2)

    def _check_cascade(self):
        if self.is_cascaded:
            raise NotImplementedError(f"{type(self).__name__}: cascade configurations (previous_stage_name) are built for "
                                      "the single-network trainers, not for the dual-branch ones")

    def set_deep_supervision_enabled(self, enabled: bool):
        self.network.do_ds = enabled  # MVDTrainer.py:802-806

    def _forward_loss(self, data, target):
        o1, o2, f1, f2 = self.network(data)
        v = self.vessel_channel
        l = self.loss(o1, target) + self.loss(o2, target)
        top1 = o1[0] if isinstance(o1, (list, tuple)) else o1
        top2 = o2[0] if isinstance(o2, (list, tuple)) else o2
        tgt0 = target[0] if isinstance(target, (list, tuple)) else target
        mutual = losses.kl_loss_compute1(top1[:, v], top2[:, v], self.kl_T)
        if self.feat_kl:
            mutual = mutual + losses.l2_loss(f1, f2, channel_wise=True, T=self.kl_T)
        l = l + self.lambda1 * mutual
        if self.use_topo and self.topo_term == 'cubical':
            tmask = ops.label_mask(tgt0, v).reshape(top1[:, v].shape)
            # the raw logit channel, as MVDTrainer.py:907 passes it; fp32 also under bf16 networks
            lt = losses.CubicalWassersteinLoss(self.topo_feat_d, self.topo_q)(top1[:, v].float(), tmask)
            self.last_cubical = lt.detach()
            l = l + self.lambda3 * lt
            if self.topo_cc:
                with torch.no_grad():
                    prob = ops.SoftmaxSelectFn.apply(top1, v)
                    self.last_topology = self._component_counts(prob, tmask.reshape(prob.shape))
        elif self.use_topo:
            if self.topo_term != 'cldice':
                raise ValueError(f"topo_term must be 'cldice' or 'cubical' (got {self.topo_term!r})")
            prob = ops.SoftmaxSelectFn.apply(top1, v)
            tmask = ops.label_mask(tgt0, v).reshape(prob.shape)
            l = l + self.lambda3 * losses.soft_cldice(prob, tmask, self.skel_iter)
            if self.topo_cc:
                self.last_topology = self._component_counts(prob.detach(), tmask)
        return l, o1

    def _graph_allowed(self):
        if self.use_topo and self.topo_term == 'cubical':
            if self.use_hip_graph:
                raise RuntimeError(f"{type(self).__name__}: topo_term = 'cubical' with use_hip_graph = True, but the step cannot "
                                   "be captured: the persistence pairing runs on the host between a D2H and an H2D copy.  Set "
                                   "use_hip_graph = False")
            return False
        return super()._graph_allowed()

    def _component_counts(self, prob, tmask):
        """The integer topology step of configs[3] ("cfg 3 + soft-clDice + CC count"; the reference's
        per-step cubical-complex pass MVDTrainer.py:907-923 runs on the CPU): number of connected components (= Betti-0,
        26-connectivity: voxels as closed top-dimensional cells) of the predicted vessel mask {softmax >= 0.5} and of the
        label's vessel mask, per sample, on the device (mvd_cc_label: union-find, bit-exact against oracle/cc_oracle.c).
        Stays on the device (no sync): {'cc_pred', 'cc_true', 'betti0_error'} int32 [N]."""
        N = prob.shape[0]
        cp, ct = [], []
        for n in range(N):
            cp.append(ops.cc_label(ops.threshold_mask(prob[n, 0], 0.5, ge=True), 26)[1])
            ct.append(ops.cc_label(ops.threshold_mask(tmask[n, 0], 0.5, ge=True), 26)[1])
        cp, ct = torch.cat(cp), torch.cat(ct)
        return {'cc_pred': cp, 'cc_true': ct, 'betti0_error': (cp - ct).abs()}

    def _graph_side_outputs(self):
        """`last_topology` of a replayed step: the graph's static tensors, overwritten by the next train step (clone
        what has to outlive it); after an eager step or a validation_step it holds that forward's own fresh tensors."""
        return self.last_topology if (self.use_topo and self.topo_cc) else None

    def _restore_graph_side_outputs(self, side):
        if side is not None:
            self.last_topology = side

    def _graph_flags(self):
        return (bool(self.network.do_ds), self.use_topo, self.topo_cc, self.skel_iter, self.feat_kl, self.kl_T,
                self.lambda1, self.lambda3, self.vessel_channel, self._label_mode())


class FinalNetTrainerMI355(ContrastiveTrainerMI355):
    """The dual-branch step on FinalNetv2 (network.MI355FinalNetv2): one encoder per modality, the two bottlenecks fused by
    cross- and self-attention, two decoders.  The network returns MVDDualBranchNet's 4-tuple, so loss, graphed step,
    validation and the optimizer paths are the parent's; fp32 only (set_precision refuses bf16 for this network)."""

    @staticmethod
    def build_network_architecture(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                   enable_deep_supervision: bool = True) -> nn.Module:
        _refuse_residual_plans(configuration_manager, "FinalNetTrainerMI355 (FinalNetv2 has plain encoders)")
        return get_finalnet_from_plans(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                       enable_deep_supervision)
