"""TEST INFRASTRUCTURE -- plain-torch 2-D PlainConvUNet with the reference's module names (the 2-D twin of
oracle/unet_oracle.py, which is 3-D only): nn.Conv2d / nn.InstanceNorm2d (or nn.BatchNorm2d) / nn.ConvTranspose2d, run in
fp64 by the tests.  The loss is oracle.loss_oracle (dimension-free); the train step is oracle.step_oracle.train_step's:
SGD-Nesterov 0.99, weight decay 3e-5, clip 12."""
import numpy as np
import torch
from torch import nn

from oracle import loss_oracle as LO
from oracle import step_oracle as SO


def _tup2(v):
    return (int(v),) * 2 if isinstance(v, (int, np.integer)) else tuple(int(i) for i in v)


class ConvDropoutNormReLU(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride, conv_bias=True, norm=nn.InstanceNorm2d, eps=1e-5, neg_slope=1e-2):
        super().__init__()
        k = _tup2(kernel_size)
        self.conv = nn.Conv2d(cin, cout, k, _tup2(stride), padding=[(i - 1) // 2 for i in k], dilation=1, bias=conv_bias)
        self.norm = norm(cout, eps=eps, affine=True)
        self.nonlin = nn.LeakyReLU(neg_slope, inplace=True)
        self.all_modules = nn.Sequential(self.conv, self.norm, self.nonlin)

    def forward(self, x):
        return self.all_modules(x)


class StackedConvBlocks(nn.Module):
    def __init__(self, num_convs, cin, cout, kernel_size, initial_stride, conv_bias=True, norm=nn.InstanceNorm2d):
        super().__init__()
        self.convs = nn.Sequential(
            ConvDropoutNormReLU(cin, cout, kernel_size, initial_stride, conv_bias, norm),
            *[ConvDropoutNormReLU(cout, cout, kernel_size, 1, conv_bias, norm) for _ in range(1, num_convs)])

    def forward(self, x):
        return self.convs(x)


class PlainConvEncoder(nn.Module):
    def __init__(self, input_channels, features, kernel_sizes, strides, n_conv, norm):
        super().__init__()
        stages, cin = [], input_channels
        for s in range(len(features)):
            stages.append(nn.Sequential(StackedConvBlocks(n_conv, cin, features[s], kernel_sizes[s], strides[s], True, norm)))
            cin = features[s]
        self.stages = nn.Sequential(*stages)
        self.output_channels = list(features)
        self.strides = [_tup2(i) for i in strides]
        self.kernel_sizes = [_tup2(k) for k in kernel_sizes]

    def forward(self, x):
        ret = []
        for s in self.stages:
            x = s(x)
            ret.append(x)
        return ret


class UNetDecoder(nn.Module):
    def __init__(self, encoder, num_classes, n_conv, deep_supervision, norm):
        super().__init__()
        self.deep_supervision = deep_supervision
        self.encoder = encoder
        stages, transpconvs, seg_layers = [], [], []
        for s in range(1, len(encoder.output_channels)):
            below, skip, st = encoder.output_channels[-s], encoder.output_channels[-(s + 1)], encoder.strides[-s]
            transpconvs.append(nn.ConvTranspose2d(below, skip, st, st, bias=True))
            stages.append(StackedConvBlocks(n_conv, 2 * skip, skip, encoder.kernel_sizes[-(s + 1)], 1, True, norm))
            seg_layers.append(nn.Conv2d(skip, num_classes, 1, 1, 0, bias=True))
        self.stages = nn.ModuleList(stages)
        self.transpconvs = nn.ModuleList(transpconvs)
        self.seg_layers = nn.ModuleList(seg_layers)

    def forward(self, skips):
        x, outs = skips[-1], []
        for s in range(len(self.stages)):
            x = self.stages[s](torch.cat((self.transpconvs[s](x), skips[-(s + 2)]), 1))
            if self.deep_supervision:
                outs.append(self.seg_layers[s](x))
            elif s == len(self.stages) - 1:
                outs.append(self.seg_layers[-1](x))
        outs = outs[::-1]
        return outs if self.deep_supervision else outs[0]


class PlainConvUNet2d(nn.Module):
    def __init__(self, input_channels, features, kernel_sizes, strides, n_conv, num_classes, deep_supervision=True,
                 norm=nn.InstanceNorm2d):
        super().__init__()
        self.encoder = PlainConvEncoder(input_channels, features, kernel_sizes, strides, n_conv, norm)
        self.decoder = UNetDecoder(self.encoder, num_classes, n_conv, deep_supervision, norm)

    def forward(self, x):
        return self.decoder(self.encoder(x))


# the tiny 2-D configuration of the GPU tests: 4 stages, base 32, 2 input channels, 3 classes, patch 40 x 56, batch 3
TINY = dict(in_ch=2, classes=3, features=[32, 64, 128, 256], strides=[[1, 1], [2, 2], [2, 2], [2, 2]], patch=(40, 56),
            batch=3)


def build(in_ch=2, classes=3, features=(32, 64, 128, 256), strides=((1, 1), (2, 2), (2, 2), (2, 2)), kernel_sizes=None,
          n_conv=2, deep_supervision=True, norm=nn.InstanceNorm2d, seed=0, dtype=torch.float64):
    """He init (network_initialization.py:4-12) under a fixed CPU seed; the norm biases get small random values so that no
    gradient is zero by symmetry."""
    torch.manual_seed(seed)
    ks = kernel_sizes or [[3, 3]] * len(features)
    m = PlainConvUNet2d(in_ch, list(features), ks, [list(s) for s in strides], n_conv, classes, deep_supervision, norm)
    for mod in m.modules():
        if isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
            nn.init.kaiming_normal_(mod.weight, a=1e-2)
            nn.init.normal_(mod.bias, 0, 0.05)
        elif isinstance(mod, (nn.InstanceNorm2d, nn.BatchNorm2d)):
            nn.init.normal_(mod.weight, 1, 0.1)
            nn.init.normal_(mod.bias, 0, 0.1)
    return m.to(dtype)


def batch(cfg=TINY, seed=1234, dtype=torch.float64):
    b = SO.synthetic_batch(cfg['batch'], cfg['in_ch'], cfg['patch'], cfg['strides'], cfg['classes'], seed)
    return {'data': b['data'].to(dtype), 'target': b['target']}


def loss_fn(n_scales, batch_dice=False):
    return LO.build_loss(n_scales, batch_dice=batch_dice)


def make_optimizer(net):
    return SO.make_optimizer(net.parameters())


train_step = SO.train_step


def to3d(net2d):
    """The same network as oracle.unet_oracle's 3-D PlainConvUNet on [N,C,1,H,W]: (1,k,k) kernels, (1,s,s) strides,
    weights unsqueezed at axis 2.  For the conditioning test of this helper."""
    from oracle import unet_oracle as UO
    enc = net2d.encoder
    m = UO.PlainConvUNet(enc.stages[0][0].convs[0].conv.in_channels, len(enc.output_channels), enc.output_channels,
                         [(1,) + k for k in enc.kernel_sizes], [(1,) + s for s in enc.strides],
                         len(enc.stages[0][0].convs), net2d.decoder.seg_layers[0].out_channels,
                         len(net2d.decoder.stages[0].convs), True, net2d.decoder.deep_supervision)
    sd = {k: (v.unsqueeze(2) if v.dim() == 4 else v) for k, v in net2d.state_dict().items()}
    m = m.to(next(net2d.parameters()).dtype)
    m.load_state_dict(sd, strict=True)
    return m
