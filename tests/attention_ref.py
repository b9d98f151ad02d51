"""fp64 restatement of the fused segment of FinalNetv2.forward (nnUNet/nnunetv2/training/my_network/selfattnNet.py:917-939)
and of its parts (UNetDecoder.py:1087-1154: Cross_Attention, Self_Attention), in plain torch on the CPU.

The reference's segment cannot be executed alone (PlainConvEncoder is not vendored), so it is restated here from helpers
that tests/golden/cross_attention.npz pins: that fixture was written by the reference's own Cross_Attention / Self_Attention
class bodies (tools/make_golden.py cross_attention), and tests/test_attention_ref_host.py holds `cross_attention` and
`self_attention` below to it at 1e-12.  Every helper computes in the dtype of its inputs, so the same code run in fp32 gives
the error of torch's own fp32 evaluation: the yardstick of the GPU tests' bars (`bar`).

Dropout is restated with explicit keep masks (1 = kept): `dropout_mask` is the host form of the kernels' generator,
Philox4x64-10 with key (seed, site) and counter ((e >> 2) + 1, t, 0, 0), element e kept iff (word >> 40) 2^-24 >= p in fp32.
"""
import numpy as np
import torch

HEADS = 8
# the six nn.Dropout calls that act in FinalNetv2.forward, in the kernels' site numbering
SITE_ATTN1, SITE_ATTN2, SITE_PROJ1, SITE_PROJ2, SITE_SELF1, SITE_SELF2 = range(6)

_M0, _M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
_W0, _W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
_MASK32 = np.uint64(0xFFFFFFFF)


def _mulhilo(a, b):
    """(high, low) 64-bit halves of the 128-bit product of the uint64 constant a and the uint64 array b."""
    a = np.uint64(a)
    a0, a1 = a & _MASK32, a >> np.uint64(32)
    b0, b1 = b & _MASK32, b >> np.uint64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p01 & _MASK32) + (p10 & _MASK32)
    hi = p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))
    return hi, a * b


def philox4x64_10(c0, c1, k0, k1):
    """Philox4x64-10 of the counters (c0[i], c1, 0, 0) under key (k0, k1): uint64 [len(c0), 4]."""
    with np.errstate(over='ignore'):
        c = [np.asarray(c0, dtype=np.uint64).copy(), np.full(len(c0), c1, dtype=np.uint64),
             np.zeros(len(c0), dtype=np.uint64), np.zeros(len(c0), dtype=np.uint64)]
        k0, k1 = np.uint64(k0), np.uint64(k1)
        for r in range(10):
            if r:
                k0, k1 = k0 + np.uint64(_W0), k1 + np.uint64(_W1)
            hi0, lo0 = _mulhilo(_M0, c[0])
            hi1, lo1 = _mulhilo(_M1, c[2])
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        return np.stack(c, axis=1)


def dropout_words(seed, t, site, n):
    """The 64-bit word of elements 0..n-1 of (seed, t, site)."""
    blocks = (n + 3) // 4
    w = philox4x64_10(np.arange(1, blocks + 1, dtype=np.uint64), t, seed, site)
    return w.reshape(-1)[:n]


def dropout_mask(seed, t, site, p, n):
    """uint8 [n], 1 = kept: (word >> 40) 2^-24 >= p, compared in fp32 as the kernels do."""
    u = (dropout_words(seed, t, site, n) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).astype(np.uint8)


def drop_scale(p):
    """1 / (1 - p) as the kernels form it (fp32)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ------------------------------------------------------------------------------------------------ parts
def layernorm(x, gamma, beta, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def linear(x, w, b=None):
    y = x @ w.t()
    return y + b if b is not None else y


def _drop(x, mask, p):
    """nn.Dropout with an explicit keep mask (None: eval mode / p = 0)."""
    if mask is None:
        return x
    return x * mask.to(x.dtype).reshape(x.shape) * drop_scale(p)


def split_heads(qkv, heads=HEADS):
    """UNetDecoder.py:1106: [B, N, 3C] -> q, k, v of [B, heads, N, dh]; channel = which C + head dh + j."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    t = qkv.reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def mha(qkv_q, qkv_kv, heads=HEADS, mask=None, p=0.0):
    """UNetDecoder.py:1111-1115: queries of the first buffer, keys / values of the second -> [B, N, C]."""
    B, N, C3 = qkv_q.shape
    q, _, _ = split_heads(qkv_q, heads)
    _, k, v = split_heads(qkv_kv, heads)
    scale = (C3 // 3 // heads) ** -0.5
    attn = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    attn = _drop(attn, mask, p)
    return (attn @ v).transpose(1, 2).reshape(B, N, C3 // 3)


def cross_attention(x1, x2, qkv1_w, qkv2_w, proj1_w, proj1_b, proj2_w, proj2_b, heads=HEADS, masks=None, p_attn=0.0,
                    p_proj=0.0):
    """Cross_Attention.forward (UNetDecoder.py:1103-1126).  masks: {site: keep mask} or None."""
    m = masks or {}
    qkv1, qkv2 = linear(x1, qkv1_w), linear(x2, qkv2_w)
    o1 = _drop(linear(mha(qkv1, qkv2, heads, m.get(SITE_ATTN1), p_attn), proj1_w, proj1_b), m.get(SITE_PROJ1), p_proj)
    o2 = _drop(linear(mha(qkv2, qkv1, heads, m.get(SITE_ATTN2), p_attn), proj2_w, proj2_b), m.get(SITE_PROJ2), p_proj)
    return o1, o2


def self_attention(x, qkv_w, heads=HEADS, mask=None, p=0.0):
    """Self_Attention.forward (UNetDecoder.py:1141-1154): the tensor BEFORE proj is returned, so proj does not enter."""
    qkv = linear(x, qkv_w)
    return mha(qkv, qkv, heads, mask, p)


FUSION_KEYS = ("pos_embed1", "pos_embed2", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "norm3.weight",
               "norm3.bias", "norm4.weight", "norm4.bias", "crossattn.qkv1.weight", "crossattn.qkv2.weight",
               "crossattn.proj1.weight", "crossattn.proj1.bias", "crossattn.proj2.weight", "crossattn.proj2.bias",
               "selfattn1.qkv.weight", "selfattn2.qkv.weight")


def fusion_block(x1, x2, P, heads=HEADS, masks=None, p_attn=0.0, p_proj=0.0, eps=1e-5):
    """selfattnNet.py:917-939 on tokens x1, x2 [B, N, C]; P: {state_dict key: tensor} over FUSION_KEYS -> (y1, y2)."""
    m = masks or {}
    x1 = x1 + P["pos_embed1"]                                                      # :924
    x2 = x2 + P["pos_embed2"]                                                      # :925
    a1, a2 = cross_attention(layernorm(x2, P["norm1.weight"], P["norm1.bias"], eps),
                             layernorm(x1, P["norm2.weight"], P["norm2.bias"], eps),
                             P["crossattn.qkv1.weight"], P["crossattn.qkv2.weight"], P["crossattn.proj1.weight"],
                             P["crossattn.proj1.bias"], P["crossattn.proj2.weight"], P["crossattn.proj2.bias"], heads, m,
                             p_attn, p_proj)                                       # :929
    a1 = a1 + x2                                                                   # :930
    y1 = x1 + self_attention(layernorm(a1, P["norm3.weight"], P["norm3.bias"], eps), P["selfattn1.qkv.weight"], heads,
                             m.get(SITE_SELF1), p_attn)                            # :931-932
    a2 = a2 + x1                                                                   # :934
    y2 = x2 + self_attention(layernorm(a2, P["norm4.weight"], P["norm4.bias"], eps), P["selfattn2.qkv.weight"], heads,
                             m.get(SITE_SELF2), p_attn)                            # :935-936
    return y1, y2


def fusion_mask_shapes(B, N, C, heads=HEADS):
    """Element counts / shapes of the six dropout sites."""
    a, pr = (B, heads, N, N), (B, N, C)
    return {SITE_ATTN1: a, SITE_ATTN2: a, SITE_PROJ1: pr, SITE_PROJ2: pr, SITE_SELF1: a, SITE_SELF2: a}


# ------------------------------------------------------------------------------------------------ bars
def bar(ref64, val32):
    """The bar of a GPU comparison against fp64: 4 x the error of torch's own fp32 CPU run of the same restatement (a
    different summation order), at least 2^-22 max|ref| (half an fp32 ulp of the largest value, twice), at most the
    project's 1e-4 max|ref|."""
    ref64 = ref64.double()
    scale = float(ref64.abs().max())
    e32 = float((val32.double() - ref64).abs().max())
    return min(max(4.0 * e32, 2.0 ** -22 * scale), 1e-4 * scale), e32


def run_both(fn, inputs, grad_outputs=None):
    """fn(*tensors) -> tensor or tuple, evaluated in fp64 and in fp32 on the CPU with gradients of every input that is a
    floating tensor: -> (outs64, grads64, outs32, grads32)."""
    res = []
    for dt in (torch.float64, torch.float32):
        ins = [t.detach().to(dt).requires_grad_(True) if torch.is_tensor(t) and t.is_floating_point() else t for t in inputs]
        outs = fn(*ins)
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        grads = None
        if grad_outputs is not None:
            leaves = [t for t in ins if torch.is_tensor(t) and t.requires_grad]
            g = torch.autograd.grad(outs, leaves, [go.to(dt) for go in grad_outputs], allow_unused=True)
            grads = [gi if gi is not None else torch.zeros_like(l) for gi, l in zip(g, leaves)]
        res += [[o.detach() for o in outs], grads]
    return res
