"""TEST INFRASTRUCTURE: a plain-torch ResidualEncoderUNet and the shared references of the residual-encoder tests.

dynamic_network_architectures (the package get_network_from_plans.py:36 takes the class from) is not vendored in the
reference, so the structure is restated here on top of oracle.unet_oracle's classes (that file is not edited): a stem of
one conv block, per stage a stack of BasicBlockD -- conv1 (conv, norm, LeakyReLU), conv2 (conv, norm), + skip, LeakyReLU; skip
= identity, or Sequential(AvgPool(stride) when strided, 1x1x1 conv (no bias) + norm when the channels change) -- and the
plain decoder.  A 2-D network is this one on [N,C,1,H,W] with (1,k,k) kernels and (1,s,s) strides (as unet2d_ref.to3d)."""
import functools

import torch
from torch import nn

from oracle import unet_oracle as UO

STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
FEATURES = [32, 64, 128]
BLOCKS = (1, 2, 2)
IN_CH, CLASSES, PATCH, BATCH = 4, 5, (16, 16, 16), 2
DATASET_JSON = {"channel_names": {str(i): f"m{i}" for i in range(IN_CH)},
                "labels": {"background": 0, "a": 1, "b": 2, "c": 3, "d": 4}}
# chosen as bn_ref's pair is (tests/bn_ref.py): among 36 (network, batch) seed pairs -- choose_seeds() below -- the one
# whose pre-activations within 5e-6 of zero carry the smallest gradients over the three steps, i.e. where a LeakyReLU branch
# that rounds the other way than in fp64 moves a gradient least
# (choose_seeds() scores, summed |gradient| in the band: (3, 5) 4.863e-3, runner-up (4, 3) 5.112e-3, then (0, 0) 6.047e-3;
# bn_ref's own pair (0, 5) scores 7.369e-3 on this network)
NET_SEED, BATCH_SEED = 3, 5


class ConvNorm(nn.Module):
    """ConvDropoutNormReLU(nonlin=None) of the package: conv2 and the skip projection."""

    def __init__(self, cin, cout, kernel_size, stride, conv_bias=True, eps=1e-5):
        super().__init__()
        k = UO._tup3(kernel_size)
        self.conv = nn.Conv3d(cin, cout, k, UO._tup3(stride), padding=[(i - 1) // 2 for i in k], dilation=1, bias=conv_bias)
        self.norm = nn.InstanceNorm3d(cout, eps=eps, affine=True)
        self.all_modules = nn.Sequential(self.conv, self.norm)

    def forward(self, x):
        return self.all_modules(x)


class BasicBlockD(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride, conv_bias=True):
        super().__init__()
        stride = UO._tup3(stride)
        self.conv1 = UO.ConvDropoutNormReLU(cin, cout, kernel_size, stride, conv_bias)
        self.conv2 = ConvNorm(cout, cout, kernel_size, 1, conv_bias)
        self.nonlin2 = nn.LeakyReLU(1e-2, inplace=True)
        ops = []
        if any(s != 1 for s in stride):
            ops.append(nn.AvgPool3d(stride, stride))
        if cin != cout:
            ops.append(ConvNorm(cin, cout, 1, 1, False))
        self.skip = nn.Sequential(*ops) if ops else nn.Identity()

    def forward(self, x):
        return self.nonlin2(self.conv2(self.conv1(x)) + self.skip(x))


class StackedResidualBlocks(nn.Module):
    def __init__(self, n_blocks, cin, cout, kernel_size, initial_stride, conv_bias=True):
        super().__init__()
        self.blocks = nn.Sequential(BasicBlockD(cin, cout, kernel_size, initial_stride, conv_bias),
                                    *[BasicBlockD(cout, cout, kernel_size, 1, conv_bias) for _ in range(1, n_blocks)])

    def forward(self, x):
        return self.blocks(x)


class ResidualEncoder(nn.Module):
    def __init__(self, input_channels, n_stages, features_per_stage, kernel_sizes, strides, n_blocks_per_stage, conv_bias=True,
                 stem_channels=None):
        super().__init__()
        stem_channels = stem_channels or features_per_stage[0]
        self.stem = UO.StackedConvBlocks(1, input_channels, stem_channels, kernel_sizes[0], 1, conv_bias)
        stages, cin = [], stem_channels
        for s in range(n_stages):
            stages.append(StackedResidualBlocks(n_blocks_per_stage[s], cin, features_per_stage[s], kernel_sizes[s], strides[s],
                                                conv_bias))
            cin = features_per_stage[s]
        self.stages = nn.Sequential(*stages)
        self.output_channels = list(features_per_stage)
        self.strides = [UO._tup3(i) for i in strides]
        self.kernel_sizes = [UO._tup3(k) for k in kernel_sizes]
        self.conv_bias = conv_bias
        self.return_skips = True

    def forward(self, x):
        x = self.stem(x)
        ret = []
        for s in self.stages:
            x = s(x)
            ret.append(x)
        return ret


class ResidualEncoderUNet(nn.Module):
    def __init__(self, input_channels, n_stages, features_per_stage, kernel_sizes, strides, n_blocks_per_stage, num_classes,
                 n_conv_per_stage_decoder, conv_bias=True, deep_supervision=True, stem_channels=None):
        super().__init__()
        self.encoder = ResidualEncoder(input_channels, n_stages, features_per_stage, kernel_sizes, strides, n_blocks_per_stage,
                                       conv_bias, stem_channels)
        self.decoder = UO.UNetDecoder(self.encoder, num_classes, n_conv_per_stage_decoder, deep_supervision)

    def forward(self, x):
        return self.decoder(self.encoder(x))


def init_last_bn_before_add_to_0(module):
    if isinstance(module, BasicBlockD):
        nn.init.constant_(module.conv2.norm.weight, 0)
        nn.init.constant_(module.conv2.norm.bias, 0)


def build(in_ch=IN_CH, classes=CLASSES, features=FEATURES, strides=STRIDES, blocks=BLOCKS, n_conv_decoder=1, kernel_sizes=None,
          deep_supervision=True, seed=NET_SEED, zero_init=True):
    """get_network_from_plans.py:15-92 restated for ResidualEncoderUNet: He init under a fixed CPU seed, then the norm in
    front of each add at zero (:90-91).  zero_init=False: every norm gets non-trivial affine parameters instead
    (randomize_norms), so that the residual branch carries signal and gradient."""
    n = len(features)
    torch.manual_seed(seed)
    m = ResidualEncoderUNet(in_ch, n, list(features), kernel_sizes or [[3, 3, 3]] * n, strides, list(blocks), classes,
                            [n_conv_decoder] * (n - 1) if isinstance(n_conv_decoder, int) else list(n_conv_decoder), True,
                            deep_supervision)
    m.apply(UO.InitWeights_He(1e-2))
    m.apply(init_last_bn_before_add_to_0)
    return m if zero_init else randomize_norms(m)


def randomize_norms(net, seed=7):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.InstanceNorm3d):
                C = m.num_features
                m.weight.copy_((torch.rand(C, generator=g) * 0.5 + 0.75).to(m.weight.dtype))
                m.bias.copy_((torch.randn(C, generator=g) * 0.1).to(m.bias.dtype))
    return net


def to2d_state_dict(sd):
    """state_dict of a (1,k,k) / (1,s,s) network -> that of the 2-D network: conv weights lose axis 2."""
    return {k: (v.squeeze(2) if v.dim() == 5 else v) for k, v in sd.items()}


def batch(seed=BATCH_SEED, patch=PATCH, strides=STRIDES):
    from oracle import step_oracle as SO
    return SO.synthetic_batch(BATCH, IN_CH, patch, strides, num_classes=CLASSES, seed=seed)


def _as(b, dtype):
    return {'data': b['data'].to(dtype), 'target': [t.to(dtype) for t in b['target']]}


def forward_backward(net, b, dtype):
    """logits, loss and every parameter gradient of one training-mode forward / backward in `dtype`."""
    from oracle import loss_oracle as LO
    net = net.to(dtype)
    b = _as(b, dtype)
    out = net(b['data'])
    l = LO.build_loss(len(b['target']))(out, b['target'])
    l.backward()
    return {'logits': [o.detach().clone() for o in out], 'loss': float(l),
            'grads': {n: p.grad.detach().clone() for n, p in net.named_parameters()}}


def evaluate(dtype, steps=3, net_seed=NET_SEED, batch_seed=BATCH_SEED):
    """bn_ref.evaluate's recipe on the residual network at its plans init (conv2.norm at zero): logits, loss and gradients of
    the first step, parameters after steps 1..`steps` of oracle/step_oracle.py (SGD lr 1e-2, weight decay 3e-5, momentum
    0.99, Nesterov, clip 12)."""
    from oracle import loss_oracle as LO, step_oracle as SO
    sd0 = {k: v.clone() for k, v in build(seed=net_seed).state_dict().items()}   # (fp32: what the HIP network loads)
    net = build(seed=net_seed).to(dtype)
    b = _as(batch(batch_seed), dtype)
    loss_fn = LO.build_loss(len(b['target']))
    opt = SO.make_optimizer(net.parameters())
    res = {'sd0': sd0, 'params': {}, 'losses': []}
    for step in range(steps):
        l, out, _gn = SO.train_step(net, loss_fn, opt, b)
        res['losses'].append(float(l))
        res['params'][step + 1] = {n: p.detach().clone() for n, p in net.named_parameters()}
    res.update(forward_backward(build(seed=net_seed), batch(batch_seed), dtype))
    return res


@functools.lru_cache(maxsize=None)
def reference64():
    """Computed once per test session, shared and left unchanged by the tests that read it."""
    return evaluate(torch.float64)


@functools.lru_cache(maxsize=None)
def reference64_random_norms():
    """One forward / backward with every norm randomised (conv2.norm away from its zero init), fp64."""
    net = build(zero_init=False)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    res = forward_backward(net, batch(), torch.float64)
    res['sd0'] = sd0
    return res


def choose_seeds(net_seeds=range(6), batch_seeds=range(6), band=5e-6, steps=3):
    """How (NET_SEED, BATCH_SEED) was chosen (not run by the tests): over the fp64 steps, the summed |gradient| that reaches
    pre-activations within `band` of zero, per seed pair; the smallest wins."""
    from oracle import loss_oracle as LO, step_oracle as SO
    score = {}
    for ns in net_seeds:
        for bs in batch_seeds:
            net = build(seed=ns).double()
            b = _as(batch(bs), torch.float64)
            loss_fn, opt = LO.build_loss(len(b['target'])), SO.make_optimizer(net.parameters())
            pre, tot = [], 0.0

            def hook(_m, inp, out):   # (the activations are in place: keep the pre-activation's value, watch the output's grad)
                out.retain_grad()
                pre.append((inp[0].detach().clone() if inp[0] is not out else None, out))

            for m in net.modules():
                if isinstance(m, nn.LeakyReLU):
                    m.inplace = False
                    m.register_forward_hook(hook)
            for _ in range(steps):
                pre.clear()
                SO.train_step(net, loss_fn, opt, b)
                tot += sum(float(y.grad[z.abs() <= band].abs().sum()) for z, y in pre if y.grad is not None)
            score[(ns, bs)] = tot
    return min(score, key=score.get), score
