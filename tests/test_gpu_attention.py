"""The kernels of csrc/attention.hip against fp64 on the CPU (tests/attention_ref.py).

Bar of every comparison (attention_ref.bar): 4 x the error of torch's own fp32 CPU run of the same restatement against
fp64, at least 2^-22 max|ref|, at most the project's 1e-4 max|ref|.
"""
import math

import numpy as np
import pytest
import torch

import attention_ref as R
from multimodal_mvd_seg_amd import network, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift).float().double()   # fp32-representable


def _gpu(t):
    return t.to(torch.float32).to(DEV).contiguous() if t is not None else None


def _check(what, got, ref64, val32):
    b, e32 = R.bar(ref64, val32)
    err = float((got.detach().cpu().double() - ref64.double()).abs().max())
    print(f"{what}: err {err:.3e}  torch-fp32 err {e32:.3e}  bar {b:.3e}  max|ref| {float(ref64.abs().max()):.3e}")
    assert err <= b, f"{what}: {err:.3e} > bar {b:.3e}"


def _state(seed=1234567, t=5):
    return torch.tensor([seed, t], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("C", [32, 64, 256, 320])
@pytest.mark.parametrize("M", [1, 3, 130])
def test_layernorm(M, C, with_pos):
    B = 2 if with_pos and M % 2 == 0 else 1
    N = M // B
    x, gam, bet = _rand(B, N, C, seed=1), _rand(C, seed=2, shift=1.0), _rand(C, seed=3)
    pos = _rand(1, N, C, seed=4) if with_pos else None
    dy, dr1 = _rand(B, N, C, seed=5), _rand(B, N, C, seed=6)

    def f(x, gam, bet, *pos):
        xs = x + pos[0] if pos else x
        return R.layernorm(xs, gam, bet), xs
    ins = [x, gam, bet] + ([pos] if with_pos else [])
    o64, g64, o32, g32 = R.run_both(f, ins, [dy, dr1])
    y, xs, mean, rstd = ops.layernorm_fwd(_gpu(x), _gpu(gam), _gpu(bet), 1e-5, _gpu(pos))
    _check("y", y, o64[0], o32[0])
    _check("xs", xs, o64[1], o32[1])
    dx, _, dg, db, dpos = ops.layernorm_bwd(_gpu(dy), xs, mean, rstd, _gpu(gam), _gpu(dr1), npos=N if with_pos else 0)
    for name, got, i in (("dx", dx, 0), ("dgamma", dg, 1), ("dbeta", db, 2)) + ((("dpos", dpos, 3),) if with_pos else ()):
        _check(name, got.reshape(g64[i].shape), g64[i], g32[i])


def test_layernorm_mean_100_std_1():
    """E[x^2] - E[x]^2 in fp32 loses the variance of such a row; the centred second pass does not."""
    x, gam, bet = _rand(3, 320, seed=7, shift=100.0), _rand(320, seed=8, shift=1.0), _rand(320, seed=9)
    dy = _rand(3, 320, seed=10)
    o64, g64, o32, g32 = R.run_both(lambda x, g, b: R.layernorm(x, g, b), [x, gam, bet], [dy])
    y, xs, mean, rstd = ops.layernorm_fwd(_gpu(x), _gpu(gam), _gpu(bet), 1e-5)
    _check("y(mean 100)", y, o64[0], o32[0])
    dx, _, dg, db, _ = ops.layernorm_bwd(_gpu(dy), xs, mean, rstd, _gpu(gam))
    _check("dx(mean 100)", dx, g64[0], g32[0])
    assert abs(float(x.mean()) - 100) < 0.5 and abs(float(x.std()) - 1) < 0.1


# ------------------------------------------------------------------------------------------------ token linear
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("C,O", [(32, 96), (320, 320), (256, 768)])
@pytest.mark.parametrize("M", [1, 27, 200, 256])
def test_linear(M, C, O, bias):
    x, w = _rand(M, C, seed=11), _rand(O, C, seed=12, scale=C ** -0.5)
    b = _rand(O, seed=13) if bias else None
    dy = _rand(M, O, seed=14)
    ins = [x, w] + ([b] if bias else [])
    o64, g64, o32, g32 = R.run_both(lambda x, w, *b: R.linear(x, w, *b), ins, [dy])
    y = ops.linear_fwd(_gpu(x), _gpu(w), _gpu(b))
    _check("y", y, o64[0], o32[0])
    dx, dw, db = ops.linear_bwd(_gpu(dy), _gpu(x), _gpu(w), has_bias=bias)
    _check("dx", dx, g64[0], g32[0])
    _check("dw", dw, g64[1], g32[1])
    if bias:
        _check("db", db, g64[2], g32[2])


@pytest.mark.parametrize("M,C,O", [(27, 32, 96), (200, 320, 320)])
def test_linear_small_integers_exact(M, C, O):
    """Integer data whose sums stay below 2^24: every fp32 product and partial sum is exact, any order."""
    g = torch.Generator().manual_seed(21)
    x = torch.randint(-4, 5, (M, C), generator=g).double()
    w = torch.randint(-4, 5, (O, C), generator=g).double()
    b = torch.randint(-4, 5, (O,), generator=g).double()
    dy = torch.randint(-4, 5, (M, O), generator=g).double()
    y = ops.linear_fwd(_gpu(x), _gpu(w), _gpu(b))
    dx, dw, db = ops.linear_bwd(_gpu(dy), _gpu(x), _gpu(w), has_bias=True)
    assert torch.equal(y.cpu().double(), x @ w.t() + b)
    assert torch.equal(dx.cpu().double(), dy @ w)
    assert torch.equal(dw.cpu().double(), dy.t() @ x)
    assert torch.equal(db.cpu().double(), dy.sum(0))


# ------------------------------------------------------------------------------------------------ attention
ATTN_SHAPES = [(1, 1, 4), (2, 27, 8), (1, 33, 40), (1, 100, 40), (2, 128, 32), (1, 256, 64)]


def _attn_case(B, N, dh, cross, scale=1.0, masks=None, p=0.0, drop=None):
    C = R.HEADS * dh
    qa = _rand(B, N, 3 * C, seed=31, scale=scale)
    qb = _rand(B, N, 3 * C, seed=32, scale=scale) if cross else None
    do = _rand(B, N, C, seed=33)
    res = _rand(B, N, C, seed=34)
    mask = None if masks is None else torch.from_numpy(masks.astype(np.float64)).reshape(B, R.HEADS, N, N)

    def f(qa, res, *qb):
        return R.mha(qa, qb[0] if qb else qa, R.HEADS, mask, p) + res
    o64, g64, o32, g32 = R.run_both(f, [qa, res] + ([qb] if cross else []), [do])
    ga = _gpu(qa)
    gb = _gpu(qb) if cross else ga
    out, mx, sm = ops.attention_fwd(ga, gb, R.HEADS, _gpu(res), drop)
    _check("out", out, o64[0], o32[0])
    dqa = torch.full_like(ga, float("nan"))
    dqb = torch.full_like(gb, float("nan")) if cross else dqa
    ops.attention_bwd(ga, gb, _gpu(do), mx, sm, R.HEADS, dqa, dqb, drop)
    if cross:   # queries of the first buffer, keys / values of the second: the other sections are not written
        _check("dq", dqa[..., :C], g64[0][..., :C], g32[0][..., :C])
        _check("dkv", dqb[..., C:], g64[2][..., C:], g32[2][..., C:])
        assert bool(torch.isnan(dqa[..., C:]).all()) and bool(torch.isnan(dqb[..., :C]).all())
    else:
        _check("dqkv", dqa, g64[0], g32[0])
    return out, mx, sm


@pytest.mark.parametrize("cross", [True, False])
@pytest.mark.parametrize("B,N,dh", ATTN_SHAPES)
def test_attention(B, N, dh, cross):
    _attn_case(B, N, dh, cross)


def test_attention_large_logits():
    """q, k scaled so that the logits reach +-60 (exp(60) = 1e26; unshifted, fp32's exp overflows from 88.7): the kernel
    exponentiates s - max <= 0 only, and the backward's recomputation uses the same saved maximum."""
    B, N, dh = 1, 33, 40
    C = R.HEADS * dh
    qa = _rand(B, N, 3 * C, seed=31, scale=3.8)
    q, k, _ = R.split_heads(qa)
    logits = (q @ k.transpose(-2, -1)) * dh ** -0.5
    assert 55 < float(logits.abs().max()) < 65, float(logits.abs().max())
    _attn_case(B, N, dh, False, scale=3.8)


def test_attention_single_token_probability_is_one():
    B, dh = 2, 4
    C = R.HEADS * dh
    qkv = _gpu(_rand(B, 1, 3 * C, seed=41, scale=5.0))
    out, mx, sm = ops.attention_fwd(qkv, qkv, R.HEADS)
    assert torch.equal(sm, torch.ones_like(sm))         # exp(0) / 1
    assert torch.equal(out, qkv[..., 2 * C:])             # probability exactly 1: the output IS v


# ------------------------------------------------------------------------------------------------ dropout
def test_dropout_p0_is_identity():
    B, N, dh = 2, 27, 8
    C = R.HEADS * dh
    st = _state()
    qkv, x, w, b = _gpu(_rand(B, N, 3 * C, seed=51)), _gpu(_rand(B * N, C, seed=52)), _gpu(_rand(C, C, seed=53)), _gpu(_rand(C, seed=54))
    assert torch.equal(ops.attention_fwd(qkv, qkv, R.HEADS, None, (st, 0.0, 0))[0], ops.attention_fwd(qkv, qkv, R.HEADS)[0])
    assert torch.equal(ops.linear_fwd(x, w, b, None, (st, 0.0, 2)), ops.linear_fwd(x, w, b))


def test_dropout_mask_matches_host_and_depends_on_t_and_site():
    seed, t, n, p = 0x1234_5678_9ABC_DEF, 9, 1 << 16, 0.1
    m = ops.dropout_mask(seed, t, 3, p, n, DEV).cpu().numpy()
    assert np.array_equal(m, R.dropout_mask(seed, t, 3, p, n))
    assert np.array_equal(m, ops.dropout_mask(seed, t, 3, p, n, DEV).cpu().numpy())
    assert not np.array_equal(m, ops.dropout_mask(seed, t + 1, 3, p, n, DEV).cpu().numpy())
    assert not np.array_equal(m, ops.dropout_mask(seed, t, 4, p, n, DEV).cpu().numpy())
    kept, sd = m.mean(), math.sqrt(0.1 * 0.9 / n)
    assert abs(kept - 0.9) <= 5 * sd, (kept, sd)


def test_dropout_tick_advances_t_only():
    st = _state(seed=77, t=5)
    ops.dropout_tick(st)
    ops.dropout_tick(st)
    assert st.cpu().tolist() == [77, 7]


def test_attention_dropout_forward_backward_regenerate_the_mask():
    B, N, dh, p, site = 2, 27, 8, 0.1, 4
    st = _state()
    seed, t = st.cpu().tolist()
    n = B * R.HEADS * N * N
    mask = ops.dropout_mask(seed, t, site, p, n, DEV).cpu().numpy()
    assert 0 < mask.sum() < n
    _attn_case(B, N, dh, True, masks=mask, p=p, drop=(st, p, site))


def test_linear_dropout_forward_backward_regenerate_the_mask():
    """proj linear with bias + dropout + residual; its backward takes the dropped gradient from the LayerNorm backward."""
    M, C, p, site = 54, 64, 0.1, 2
    st = _state()
    seed, t = st.cpu().tolist()
    mask = torch.from_numpy(ops.dropout_mask(seed, t, site, p, M * C, DEV).cpu().numpy().astype(np.float64)).reshape(M, C)
    x, w, b, res = _rand(M, C, seed=61), _rand(C, C, seed=62, scale=C ** -0.5), _rand(C, seed=63), _rand(M, C, seed=64)
    gam, bet, dy = _rand(C, seed=65, shift=1.0), _rand(C, seed=66), _rand(M, C, seed=67)

    def f(x, w, b, res, gam, bet):
        a = R._drop(R.linear(x, w, b), mask, p) + res
        return R.layernorm(a, gam, bet), a
    o64, g64, o32, g32 = R.run_both(f, [x, w, b, res, gam, bet], [dy, torch.zeros(M, C, dtype=torch.float64)])
    a = ops.linear_fwd(_gpu(x), _gpu(w), _gpu(b), _gpu(res), (st, p, site))
    _check("a", a, o64[1], o32[1])
    y, _, mean, rstd = ops.layernorm_fwd(a, _gpu(gam), _gpu(bet), 1e-5)
    _check("y", y, o64[0], o32[0])
    da, dad, dg, dbt, _ = ops.layernorm_bwd(_gpu(dy), a, mean, rstd, _gpu(gam), drop=(st, p, site))
    _check("dres", da, g64[3], g32[3])
    dx, dw, db = ops.linear_bwd(dad, _gpu(x), _gpu(w), has_bias=True)
    for name, got, i in (("dx", dx, 0), ("dw", dw, 1), ("db", db, 2)):
        _check(name, got, g64[i], g32[i])


# ------------------------------------------------------------------------------------------------ the whole block
def _block(B, sp, C, training, seed=0):
    torch.manual_seed(seed)
    N = int(np.prod(sp))
    fus = network.BottleneckFusion(C, N).to(DEV)
    with torch.no_grad():   # every parameter away from its initial value (pos 0, gamma 1, beta 0)
        g = torch.Generator().manual_seed(seed + 1)
        for p in fus.fusion_parameters():
            p.add_(torch.randn(p.shape, generator=g).to(DEV) * 0.1)
    fus.train(training)
    return fus, N


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B,sp,C", [(2, (2, 4, 4), 64), (1, (2, 8, 8), 256)])
def test_fusion_block(B, sp, C, training):
    fus, N = _block(B, sp, C, training)
    P = {k: v.detach().cpu() for k, v in fus.state_dict().items() if k in R.FUSION_KEYS}
    names = list(R.FUSION_KEYS)
    x1, x2 = _rand(B, N, C, seed=71), _rand(B, N, C, seed=72)
    dy1, dy2 = _rand(B, N, C, seed=73), _rand(B, N, C, seed=74)
    p_attn, p_proj = (0.1, 0.1) if training else (0.0, 0.0)
    masks = None
    if training:   # the step this forward will run is t + 1: the tick comes first
        seed, t = fus.mvd_dropout_state.cpu().tolist()
        masks = {s: torch.from_numpy(ops.dropout_mask(seed, t + 1, s, 0.1, int(np.prod(shp)), DEV).cpu().numpy()
                                     .astype(np.float64)).reshape(shp)
                 for s, shp in R.fusion_mask_shapes(B, N, C).items()}

    def f(x1, x2, *ps):
        return R.fusion_block(x1, x2, dict(zip(names, ps)), R.HEADS, masks, p_attn, p_proj)
    o64, g64, o32, g32 = R.run_both(f, [x1, x2] + [P[k] for k in names], [dy1, dy2])

    def run():
        as5 = lambda t: _gpu(t).view(B, *sp, C).permute(0, 4, 1, 2, 3)
        a, b = as5(x1).requires_grad_(True), as5(x2).requires_grad_(True)
        fus.zero_grad()
        y1, y2 = fus(a, b)
        torch.autograd.backward([y1, y2], [as5(dy1), as5(dy2)])
        tok = lambda t: t.permute(0, 2, 3, 4, 1).reshape(B, N, C)
        sd = dict(fus.named_parameters())
        return [tok(y1), tok(y2)], [tok(a.grad), tok(b.grad)] + [sd[k].grad for k in names]
    outs, grads = run()
    for i, o in enumerate(outs):
        _check(f"y{i + 1}", o, o64[i], o32[i])
    for name, g, r64, r32 in zip(["dx1", "dx2"] + names, grads, g64, g32):
        _check(name, g, r64, r32)
    for n_, p_ in fus.named_parameters():
        if n_ not in names:
            assert p_.grad is None and not p_.requires_grad, n_
    # a second identical run (training: the same step again) is bit-identical
    if training:
        fus.mvd_dropout_state[1] -= 1
    outs2, grads2 = run()
    for a_, b_ in zip(outs + grads, outs2 + grads2):
        assert torch.equal(a_, b_)
    if not training:
        assert fus.mvd_dropout_state.cpu().tolist()[1] == 0   # eval forwards do not advance t


# ------------------------------------------------------------------------------------------------ the stand-alone modules
def test_modules_reproduce_the_reference_fixture_and_its_gradients():
    """network.Cross_Attention / Self_Attention / HipLayerNorm called on their own (eval mode: ops.TokenLinearFn,
    ops.AttentionFn, ops.LayerNormFn) against tests/golden/cross_attention.npz, gradients against the restatement."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_attention.npz"), allow_pickle=False)
    T = lambda k: torch.from_numpy(z[k]).float().double()   # what the fp32 modules see
    C, H = 32, int(z["heads"])
    ca, sa, ln = network.Cross_Attention(C, H, False, 0.1, 0.1), network.Self_Attention(C, H, False, 0.1, 0.1), network.HipLayerNorm(C)
    ca.load_state_dict({k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("ca/")})
    sa.load_state_dict({"qkv.weight": T("sa/qkv.weight").float(), "proj.weight": T("sa/proj.weight").float(),
                        "proj.bias": T("sa/proj.bias").float()})
    for m in (ca, sa, ln):
        m.to(DEV).eval()
    ca_keys = ("qkv1.weight", "qkv2.weight", "proj1.weight", "proj1.bias", "proj2.weight", "proj2.bias")
    x1, x2, d1, d2, d3 = T("x1"), T("x2"), _rand(2, 16, C, seed=81), _rand(2, 16, C, seed=82), _rand(2, 16, C, seed=83)
    gam, bet = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)

    def f(x1, x2, saw, gam, bet, *caw):
        o1, o2 = R.cross_attention(R.layernorm(x1, gam, bet), x2, *caw, H)
        return o1, o2, R.self_attention(x1, saw, H)
    o64, g64, o32, g32 = R.run_both(f, [x1, x2, T("sa/qkv.weight"), gam, bet] + [T("ca/" + k) for k in ca_keys], [d1, d2, d3])
    a, b = _gpu(x1).requires_grad_(True), _gpu(x2).requires_grad_(True)
    o1, o2 = ca(ln(a), b)
    o3 = sa(a)
    torch.autograd.backward([o1, o2, o3], [_gpu(d1), _gpu(d2), _gpu(d3)])
    for i, o in enumerate((o1, o2, o3)):
        _check(f"module out{i}", o, o64[i], o32[i])
    # without the LayerNorm in front the fixture itself is reproduced (its inputs rounded to fp32: 1e-5 of max|ref|)
    with torch.no_grad():
        p1, p2 = ca(a, b)
    for got, key in ((p1, "ca_out1"), (p2, "ca_out2"), (o3, "sa_out")):
        want = torch.from_numpy(z[key])
        assert float((got.detach().cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max()), key
    got = [a.grad, b.grad, sa.qkv.weight.grad, ln.weight.grad, ln.bias.grad] + [dict(ca.named_parameters())[k].grad for k in ca_keys]
    for name, g, r64, r32 in zip(["dx1", "dx2", "sa.qkv", "ln.w", "ln.b"] + list(ca_keys), got, g64, g32):
        _check("module grad " + name, g, r64, r32)
    assert sa.proj.weight.grad is None   # the quirk: proj is never used
    ca.train()
    with pytest.raises(NotImplementedError, match="BottleneckFusion"):
        ca(a, b)
