"""TEST INFRASTRUCTURE: the BatchNorm3d form of the oracle network and the shared references of the BatchNorm tests.

The reference's BN trainer (variants/network_architecture/nnUNetTrainerBN.py:31-32) passes norm_op =
get_matching_batchnorm(conv_op) = torch.nn.BatchNorm3d, so torch on the CPU IS the oracle: oracle.unet_oracle's network
with every ConvDropoutNormReLU.norm replaced by nn.BatchNorm3d(cout, eps=1e-5, affine=True) (the oracle file itself is not
edited)."""
import copy
import functools

import torch
from torch import nn

STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
FEATURES = [32, 64, 128]
IN_CH, CLASSES, PATCH, BATCH = 4, 5, (16, 16, 16), 2
DATASET_JSON = {"channel_names": {str(i): f"m{i}" for i in range(IN_CH)},
                "labels": {"background": 0, "a": 1, "b": 2, "c": 3, "d": 4}}
# chosen among 48 (network, batch) seed pairs: the one whose pre-activations within 5e-6 of zero carry the smallest gradients
# over the three steps, i.e. where a LeakyReLU branch that rounds the other way than in fp64 moves a gradient least
NET_SEED, BATCH_SEED = 0, 5


def swap_to_batchnorm(net):
    """Every ConvDropoutNormReLU.norm of an oracle.unet_oracle network -> nn.BatchNorm3d; all_modules rebuilt."""
    from oracle import unet_oracle as UO
    for m in net.modules():
        if isinstance(m, UO.ConvDropoutNormReLU):
            m.norm = nn.BatchNorm3d(m.conv.out_channels, eps=1e-5, affine=True)
            m.all_modules = nn.Sequential(m.conv, m.norm, m.nonlin)
    return net


def randomize_bn(net, seed=7):
    """Non-trivial affine parameters and running buffers (a fresh BatchNorm has gamma = 1, beta = 0, mean 0, var 1, which
    hides a kernel that ignores one of them)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm3d):
                C = m.num_features
                m.weight.copy_((torch.rand(C, generator=g) * 0.5 + 0.75).to(m.weight.dtype))
                m.bias.copy_((torch.randn(C, generator=g) * 0.1).to(m.bias.dtype))
                m.running_mean.copy_((torch.randn(C, generator=g) * 0.1).to(m.running_mean.dtype))
                m.running_var.copy_((torch.rand(C, generator=g) * 0.5 + 0.75).to(m.running_var.dtype))
    return net


def bn_oracle(deep_supervision=True, seed=NET_SEED):
    """The smallest net that exercises every path: 3 stages, 32/64/128 features, 4 input channels (fp32, train mode)."""
    from oracle import unet_oracle as UO
    net = UO.build_plainconv_unet(IN_CH, CLASSES, 3, STRIDES, features_per_stage=FEATURES,
                                  deep_supervision=deep_supervision, seed=seed)
    return randomize_bn(swap_to_batchnorm(net))


def batch(seed=BATCH_SEED):
    from oracle import step_oracle as SO
    return SO.synthetic_batch(BATCH, IN_CH, PATCH, STRIDES, num_classes=CLASSES, seed=seed)


def _as(b, dtype):
    return {'data': b['data'].to(dtype), 'target': [t.to(dtype) for t in b['target']]}


def evaluate(dtype, steps=3):
    """The swapped oracle in `dtype` (fp32 or fp64) on the synthetic batch, training mode: logits, loss and every gradient
    of the first step, the buffers after it, parameters and buffers after steps 1..`steps` of the oracle/step_oracle.py
    recipe (SGD lr 1e-2, weight decay 3e-5, momentum 0.99, Nesterov, clip 12)."""
    from oracle import loss_oracle as LO, step_oracle as SO
    net = bn_oracle().to(dtype)
    sd0 = {k: v.clone() for k, v in bn_oracle().state_dict().items()}   # (fp32: what the HIP network loads)
    b = _as(batch(), dtype)
    loss_fn = LO.build_loss(len(b['target']))
    opt = SO.make_optimizer(net.parameters())
    res = {'sd0': sd0, 'params': {}, 'buffers': {}, 'losses': []}
    for step in range(steps):
        l, out, _gn = SO.train_step(net, loss_fn, opt, b)
        res['losses'].append(float(l))
        if step == 0:
            res['logits'] = [o.detach().clone() for o in out]
        res['params'][step + 1] = {n: p.detach().clone() for n, p in net.named_parameters()}
        res['buffers'][step + 1] = {n: v.detach().clone() for n, v in net.named_buffers()}
    # the gradients of the first step (train_step clips them in place: evaluate them apart, on a fresh copy)
    net = bn_oracle().to(dtype)
    l = loss_fn(net(b['data']), b['target'])
    l.backward()
    res['grads'] = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    return res


@functools.lru_cache(maxsize=None)
def reference64():
    """Computed once per test session, shared and left unchanged by the tests that read it."""
    return evaluate(torch.float64)


def grad_tol(name, ref):
    """The per-parameter bars of the tiny-U-Net test (tests/test_gpu_parity.py): the conv bias in front of a
    normalisation has an analytically zero gradient (rounding noise on both sides)."""
    tol = 2e-5 if (name.endswith("conv.bias") or "all_modules.0.bias" in name) else 1e-4
    return tol * max(1.0, float(ref.abs().max()))


def buffer_tol(ref):
    """Running buffers of a NETWORK: 2e-6 relative to the buffer's scale.  (Behind fp32 convolutions an entry that
    cancels to almost nothing cannot be held to its own size; the kernel tests, whose input is exact, hold every entry to
    2e-6 of itself.)"""
    return 2e-6 * max(1.0, float(ref.abs().max()))


def eval_oracle(deep_supervision=False):
    """The swapped oracle in eval() with the non-trivial running buffers, fp64: what the predictor is compared with."""
    net = bn_oracle(deep_supervision=deep_supervision)
    sd = copy.deepcopy(net.state_dict())
    return net.double().eval(), sd
