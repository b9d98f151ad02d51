"""GPU tests of the residual encoder: the block-tail kernels and the skip branch's pool against fp64, the network against
the fp64 torch restatement (tests/resenc_ref.py), the trainer against the stepped oracle, graph vs eager, the predictor.

Bars of the block tail: those of tests/test_gpu_instnorm_paths.py -- y within 2e-6 max(1, max|y64|), da / dr within 5e-6 of
their maxima, dgamma / dbeta within 1e-5 of theirs; the fp64 backward uses the HIP forward's LeakyReLU branches, which may
differ from sign(z64) only where |z64| <= 1e-5 (asserted)."""
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bn_ref
import resenc_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CL = torch.channels_last_3d
SLOPE, EPS = 0.01, 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def close(a, b, atol, rtol=0.0, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    print(f"{what}: max abs err {float(err.max()):.3e} at max |ref| {float(b.abs().max()):.3e} (tol {atol:g}+{rtol:g}*|ref|)")
    assert bool((err <= tol).all()), f"{what}: max abs err {float(err.max()):.3e} (tol {atol:g}+{rtol:g}*|ref|)"


# ================================================================================================ block tail
BIG_TAIL = (1, 256, (16, 16, 33))   # 132 blocks: lanes 0-3 of a finalize wave sum three partials, the rest two
TAIL_SHAPES = [(2, 32, (8, 8, 8)), (1, 64, (6, 5, 7)), (3, 5, (3, 3, 3)), (2, 320, (2, 2, 2)), (2, 32, (16, 16, 8)), BIG_TAIL]


def _tail_inputs(N, C, sp, proj, gamma_zero, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + N * 131 + C)
    t = {"a": torch.randn(N, C, *sp, generator=g) * 1.5 + 0.3, "r": torch.randn(N, C, *sp, generator=g) * 0.8 - 0.2,
         "dy": torch.randn(N, C, *sp, generator=g), "prev": torch.randn(N, C, *sp, generator=g),
         "ga": torch.rand(C, generator=g) * 0.5 + 0.75, "ba": torch.randn(C, generator=g) * 0.1}
    if gamma_zero:      # the initial state of conv2.norm (init_last_bn_before_add_to_0)
        t["ga"], t["ba"] = torch.zeros(C), torch.zeros(C)
    if proj:
        t["gr"], t["br"] = torch.rand(C, generator=g) * 0.5 + 0.75, torch.randn(C, generator=g) * 0.1
    return t


def _tail_z64(t, a, r, ga, ba, gr=None, br=None):
    z = F.instance_norm(a, weight=ga, bias=ba, eps=EPS)
    return z + (F.instance_norm(r, weight=gr, bias=br, eps=EPS) if gr is not None else r)


def _tail_hip(t, proj, accumulate):
    """(y, da, dr, dgamma_a, dbeta_a[, dgamma_r, dbeta_r]) of ops.ResidualAddNormActFn; accumulate: r carries a shared
    gradient buffer that already holds `prev`, the kernel adds dr into it."""
    from multimodal_mvd_seg_amd import ops
    G = lambda k: t[k].to(DEV).requires_grad_()
    a = t["a"].to(DEV).contiguous(memory_format=CL).requires_grad_()
    r = t["r"].to(DEV).contiguous(memory_format=CL).requires_grad_()
    ps = [G("ga"), G("ba")] + ([G("gr"), G("br")] if proj else [None, None])
    buf = None
    if accumulate:
        ops.share_grad(r)
        buf = t["prev"].to(DEV).contiguous(memory_format=CL).clone(memory_format=CL)
        r._mvd_gshare.buf = buf
    y = ops.ResidualAddNormActFn.apply(a, ps[0], ps[1], r, ps[2], ps[3], EPS, SLOPE)
    y.backward(t["dy"].to(DEV).contiguous(memory_format=CL))
    if accumulate:
        assert r.grad is None, "a joined gradient must not be returned to autograd as well"
        dr = buf                          # prev + dr
    else:
        dr = r.grad
    return [y.detach(), a.grad, dr] + [p.grad for p in ps if p is not None]


@pytest.mark.parametrize("gamma_zero", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("N,C,sp", TAIL_SHAPES)
def test_block_tail_forward_backward_vs_fp64(N, C, sp, proj, accumulate, gamma_zero):
    if (N, C, sp) == BIG_TAIL:      # (the block tail's geometry is InstanceNorm's: csrc/norm_common.h)
        from multimodal_mvd_seg_amd._lib import query
        nblk = query("mvd_instnorm_nblk", N, sp[0] * sp[1] * sp[2], C)
        assert nblk > 128, f"{nblk} block partials per sample: the two-in-flight loop of the finalize kernels is not exercised"
    t = _tail_inputs(N, C, sp, proj, gamma_zero)
    got = _tail_hip(t, proj, accumulate)
    again = _tail_hip(t, proj, accumulate)
    names = ["y", "da", "dr", "dgamma_a", "dbeta_a", "dgamma_r", "dbeta_r"]
    for n, u, v in zip(names, got, again):
        assert torch.equal(u, v), f"{n} differs between two runs"
    # fp64 reference with the HIP forward's branches
    d = {k: v.double().requires_grad_() for k, v in t.items() if k not in ("dy", "prev")}
    z64 = _tail_z64(t, d["a"], d["r"], d["ga"], d["ba"], d.get("gr"), d.get("br"))
    # (planar strides for everything that enters the fp64 graph: with a channels-last mask torch's CPU instance_norm backward
    # mis-reads the strided gradient of a one-sample batch)
    y = got[0].cpu().contiguous().double()
    # the branch the kernel took: y > 0 <=> z > 0 (slope > 0); z == 0 takes the slope as torch does
    pos = y > 0
    flips = pos != (z64.detach() > 0)
    assert not int(flips.sum()) or float(z64.detach()[flips].abs().max()) <= 1e-5, "LeakyReLU branch differs away from zero"
    y64 = torch.where(pos, z64, z64 * SLOPE)
    ymax = max(1.0, float(y64.abs().max()))
    ey = (y - y64.detach()).abs()
    print(f"y: {float(ey.max()) / ymax:.2e} of max(1, max|y64|)   (bar 2e-6)")
    assert float(ey.max()) <= 2e-6 * ymax
    y64.backward(t["dy"].double())
    ref = [None, d["a"].grad, d["r"].grad, d["ga"].grad, d["ba"].grad] + ([d["gr"].grad, d["br"].grad] if proj else [])
    for n, u, v, bar in zip(names[1:], got[1:], ref[1:], (5e-6, 5e-6, 1e-5, 1e-5, 1e-5, 1e-5)):
        m, extra = float(v.abs().max()), 0.0
        if n == "dr" and accumulate:
            # the buffer holds fl(prev + dr): the bar of dr plus the one rounding of the fp32 sum, half an ulp of its maximum
            v = v + t["prev"].double()
            extra = 2.0 ** -24 * float(v.abs().max())
        e = float((u.cpu().double() - v).abs().max())
        print(f"{n}: {e:.3e} at a maximum of {m:.3e}   (bar {bar:g} of the maximum)")
        assert e <= bar * m + extra, f"{n}: {e:.3e} vs bar {bar:g} * {m:.3e}"


def test_block_tail_refusals_launch_nothing():
    from multimodal_mvd_seg_amd import _lib, ops
    lib = _lib.load()
    x = torch.randn(16, device=DEV)
    gam, bet, mean, rstd = (torch.ones(64, device=DEV) for _ in range(4))
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    P = ops._p
    args = lambda a, r, y, N, V, C: (P(a), P(gam), P(bet), P(r), None, None, P(y), P(mean), P(rstd), None, None, N, V, C, EPS,
                                     SLOPE, 0, P(ws), ws.numel(), None)
    y = torch.full((16,), 7.0, device=DEV)
    buf = torch.zeros(4, device=DEV)
    for N, V, C in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (2, 1, 8), (-1, 8, 4)):
        assert lib.mvd_resblock_fwd(*args(x, x, y, N, V, C)) != 0, (N, V, C)
        assert len(lib.mvd_last_error()) > 10
    off = torch.zeros(65, device=DEV)[1:]            # 4-byte aligned only
    assert lib.mvd_resblock_fwd(*args(off, x, y, 2, 2, 4)) != 0 and b"aligned" in lib.mvd_last_error()
    assert lib.mvd_resblock_fwd(*args(x, x, off, 2, 2, 4)) != 0 and b"aligned" in lib.mvd_last_error()
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(y.max()) == 7.0 and float(off.abs().max()) == 0.0
    assert lib.mvd_resblock_fwd(*args(off, x, off[16:], 2, 2, 3)) == 0   # C % 4 != 0: the scalar path has no requirement
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="ResidualEncoderUNet"):
        h = torch.zeros(1, 4, 2, 2, 2, device=DEV, dtype=torch.bfloat16)
        ops.ResidualAddNormActFn.apply(h, buf, buf, h, None, None, EPS, SLOPE)


def test_block_tail_backward_refusals_launch_nothing():
    from multimodal_mvd_seg_amd import _lib, ops
    lib = _lib.load()
    P = ops._p
    x = torch.randn(16, device=DEV)
    gam, bet, mean, rstd = (torch.ones(64, device=DEV) for _ in range(4))
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    da, dr, dg, db = (torch.full((16,), 7.0, device=DEV) for _ in range(4))
    off = torch.zeros(65, device=DEV)[1:]            # 4-byte aligned only

    def call(N, V, C, a=x, r=x, dy=x, da_=da, dr_=dr, gr=None, br=None, mr=None, sr=None, dgr=None, dbr=None):
        return lib.mvd_resblock_bwd(P(a), P(r), P(dy), P(gam), P(bet), P(mean), P(rstd), P(gr), P(br), P(mr), P(sr), P(da_),
                                    P(dr_), P(dg), P(db), P(dgr), P(dbr), 0, N, V, C, SLOPE, P(ws), ws.numel(), None)

    for N, V, C in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (2, 1, 8), (-1, 8, 4)):
        assert call(N, V, C) != 0, (N, V, C)
        assert len(lib.mvd_last_error()) > 10
    for kw in (dict(a=off), dict(r=off), dict(dy=off), dict(da_=off), dict(dr_=off)):
        assert call(2, 2, 4, **kw) != 0 and b"aligned" in lib.mvd_last_error(), kw
    # the projection form needs all of beta_r, mean_r, rstd_r, dgamma_r, dbeta_r
    full = dict(gr=gam, br=bet, mr=mean, sr=rstd, dgr=dg, dbr=db)
    for drop in ("br", "mr", "sr", "dgr", "dbr"):
        assert call(2, 2, 4, **{k: v for k, v in full.items() if k != drop}) != 0, drop
        assert b"projection" in lib.mvd_last_error()
    small = torch.zeros(8, dtype=torch.uint8, device=DEV)
    assert lib.mvd_resblock_bwd(P(x), P(x), P(x), P(gam), P(bet), P(mean), P(rstd), None, None, None, None, P(da), P(dr), P(dg),
                                P(db), None, None, 0, 2, 2, 4, SLOPE, P(small), small.numel(), None) != 0
    assert b"workspace" in lib.mvd_last_error()
    torch.cuda.synchronize()
    for t in (da, dr, dg, db):
        assert float(t.min()) == 7.0 and float(t.max()) == 7.0
    assert float(off.abs().max()) == 0.0


@pytest.mark.parametrize("N,C,sp", [(2, 32, (16, 16, 8)), (3, 5, (3, 3, 3))])
def test_block_tail_takes_precomputed_statistics(N, C, sp):
    """have_stats: bit 0 / bit 1 say that mean / rstd of a / of r were filled by the caller (from a conv's tile statistics);
    the kernel then skips that tensor's statistics pass.  Given the statistics it would compute itself, every combination
    returns the same y bit for bit, leaves the given pair alone and fills the other one.  have_stats = 1 in the projection
    form is the statistics launch over r alone."""
    from multimodal_mvd_seg_amd import _lib, ops
    lib = _lib.load()
    P = ops._p
    t = _tail_inputs(N, C, sp, True, False)
    V = sp[0] * sp[1] * sp[2]
    a, r = (t[k].to(DEV).contiguous(memory_format=CL) for k in ("a", "r"))
    ga, ba, gr, br = (t[k].to(DEV) for k in ("ga", "ba", "gr", "br"))
    ws = torch.zeros(max(lib.mvd_resblock_workspace_bytes(N, V, C), 1 << 16), dtype=torch.uint8, device=DEV)

    def run(proj, have, given=None):
        y = torch.empty_like(a)
        st = [torch.full((N, C), float("nan"), device=DEV) for _ in range(4)]      # mean_a, rstd_a, mean_r, rstd_r
        if given is not None:
            for i in ((0, 1) if have & 1 else ()) + ((2, 3) if have & 2 else ()):
                st[i] = given[i].clone()
        rc = lib.mvd_resblock_fwd(P(a), P(ga), P(ba), P(r), P(gr) if proj else None, P(br) if proj else None, P(y), P(st[0]),
                                  P(st[1]), P(st[2]) if proj else None, P(st[3]) if proj else None, N, V, C, EPS, SLOPE, have,
                                  P(ws), ws.numel(), None)
        assert rc == 0, lib.mvd_last_error()
        torch.cuda.synchronize()
        return y, st

    for proj, haves in ((False, (1,)), (True, (1, 2, 3))):
        y0, st0 = run(proj, 0)
        assert not any(bool(torch.isnan(s).any()) for s in (st0 if proj else st0[:2]))
        for have in haves:
            y, st = run(proj, have, st0)
            assert torch.equal(y, y0), (proj, have)
            for s, s0 in zip(st if proj else st[:2], st0):
                assert torch.equal(s, s0), (proj, have)


# ================================================================================================ pool
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("stride", [(2, 2, 2), (1, 2, 2), (2, 2, 1)])
@pytest.mark.parametrize("N,C,sp", [(2, 32, (8, 8, 8)), (1, 5, (4, 6, 2)), (2, 320, (2, 2, 2))])
def test_avgpool_vs_torch_fp64(N, C, sp, stride, accumulate):
    from multimodal_mvd_seg_amd import ops
    g = torch.Generator().manual_seed(N * 100 + C)
    x = torch.randint(-64, 64, (N, C, *sp), generator=g).float()      # integer-valued: the average of <= 8 is exact in fp32
    osp = [e // s for e, s in zip(sp, stride)]
    dy = torch.randint(-64, 64, (N, C, *osp), generator=g).float()
    prev = torch.randint(-64, 64, (N, C, *sp), generator=g).float()
    x64 = x.double().requires_grad_()
    y64 = F.avg_pool3d(x64, stride, stride)
    y64.backward(dy.double())
    outs = []
    for _ in range(2):
        xg = x.to(DEV).contiguous(memory_format=CL).requires_grad_()
        buf = None
        if accumulate:
            ops.share_grad(xg)
            buf = prev.to(DEV).contiguous(memory_format=CL).clone(memory_format=CL)
            xg._mvd_gshare.buf = buf
        y = ops.AvgPool3dFn.apply(xg, stride)
        assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == tuple(y64.shape)
        y.backward(dy.to(DEV).contiguous(memory_format=CL))
        if accumulate:
            assert xg.grad is None
        outs.append((y.detach().cpu(), (buf if accumulate else xg.grad).cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    y, dx = outs[0]
    dx64 = x64.grad + (prev.double() if accumulate else 0)
    # 1 ulp of fp32 is the bar; with integer-valued inputs every value is exact, so the results are equal bit for bit
    assert bool(((y.double() - y64.detach()).abs() <= 2.0 ** -23 * y64.detach().abs()).all())
    assert torch.equal(y.double(), y64.detach()), "y"
    assert bool(((dx.double() - dx64).abs() <= 2.0 ** -23 * dx64.abs()).all())
    assert torch.equal(dx.double(), dx64), "dx"


def test_avgpool_odd_extent_is_refused_and_launches_nothing():
    from multimodal_mvd_seg_amd import _lib, ops
    lib = _lib.load()
    x = torch.randn(1, 8, 5, 4, 4, device=DEV).contiguous(memory_format=CL)
    y = torch.full((1, 8, 2, 2, 2), 7.0, device=DEV).contiguous(memory_format=CL)
    P, i3 = ops._p, _lib.i3
    assert lib.mvd_avgpool3d_fwd(P(x), P(y), 1, 5, 4, 4, 8, i3((2, 2, 2)), None) != 0
    assert b"odd extent" in lib.mvd_last_error()
    assert lib.mvd_avgpool3d_bwd(P(y), P(x), 1, 5, 4, 4, 8, i3((2, 2, 2)), 0, None) != 0
    assert lib.mvd_avgpool3d_fwd(P(x), P(y), 1, 5, 4, 4, 8, i3((1, 3, 2)), None) != 0      # stride 3
    assert lib.mvd_avgpool3d_fwd(P(x), P(y), 0, 4, 4, 4, 8, i3((2, 2, 2)), None) != 0
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(y.max()) == 7.0
    with pytest.raises(RuntimeError, match="odd extent"):
        ops.AvgPool3dFn.apply(x, (2, 2, 2))
    y122 = torch.empty(1, 8, 5, 2, 2, device=DEV).contiguous(memory_format=CL)               # the output of stride (1, 2, 2)
    assert lib.mvd_avgpool3d_fwd(P(x), P(y122), 1, 5, 4, 4, 8, i3((1, 2, 2)), None) == 0   # the odd axis is not strided
    torch.cuda.synchronize()
    assert torch.allclose(y122, F.avg_pool3d(x, (1, 2, 2), (1, 2, 2)), rtol=1e-6, atol=1e-6)


# ================================================================================================ network
def _hip_net(sd, conv_op=nn.Conv3d, strides=resenc_ref.STRIDES, deep_supervision=True):
    from multimodal_mvd_seg_amd import network
    norm = nn.InstanceNorm3d if conv_op is nn.Conv3d else nn.InstanceNorm2d
    net = network.MI355ResidualEncoderUNet(resenc_ref.IN_CH, 3, resenc_ref.FEATURES, conv_op, 3, strides, resenc_ref.BLOCKS,
                                           resenc_ref.CLASSES, 1, True, norm, {'eps': 1e-5, 'affine': True}, None, None,
                                           nn.LeakyReLU, {'inplace': True}, deep_supervision=deep_supervision)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


def _gbatch(b):
    return {"data": b["data"].to(DEV), "target": [t.to(DEV) for t in b["target"]]}


def _loss(n_scales):
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(resenc_ref.PATCH, resenc_ref.STRIDES, batch_size=resenc_ref.BATCH,
                               unet_class_name='ResidualEncoderUNet', n_blocks_per_stage=resenc_ref.BLOCKS,
                               n_conv_per_stage_decoder=(1, 1))
    tr = trainer.nnUNetTrainerMI355(plans, "3d_fullres", 0, resenc_ref.DATASET_JSON, device=DEV)
    return tr._build_loss()


def _check_fwd_bwd(net, gb, r, squeeze=False):
    out = net(gb["data"])
    l = _loss(len(out))(out, gb["target"])
    l.backward()
    for i, (o, ref) in enumerate(zip(out, r['logits'])):
        assert o.dtype == torch.float32
        close(o, ref.squeeze(2) if squeeze else ref, 1e-4, 0, f"logits{i}")
    assert abs(float(l) - r['loss']) <= 1e-5 * max(1.0, abs(r['loss'])), (float(l), r['loss'])
    for n, p in net.named_parameters():
        ref = r['grads'][n]
        ref = ref.squeeze(2) if (squeeze and ref.dim() == 5) else ref
        assert p.grad is not None, n
        close(p.grad, ref, bn_ref.grad_tol(n, ref), 0, "grad " + n)


@pytest.mark.parametrize("zero_init", [True, False])
def test_network_matches_the_fp64_restatement(zero_init):
    r = resenc_ref.reference64() if zero_init else resenc_ref.reference64_random_norms()
    net = _hip_net(r['sd0'])
    # interchange, the other direction: our state_dict loads into the restatement, strictly
    resenc_ref.build().load_state_dict({k: v.cpu() for k, v in net.state_dict().items()}, strict=True)
    _check_fwd_bwd(net, _gbatch(resenc_ref.batch()), r)
    if not zero_init:   # the residual branch carries gradient: conv2 and its norm are not at rest
        assert float(net.encoder.stages[1].blocks[1].conv2.conv.weight.grad.abs().max()) > 0


def test_network_with_a_projection_only_skip_on_a_decoder_skip_matches_fp64():
    """Strides 1/1/2 with 32/64/128 features: stage 1 changes channels at stride 1, so its first block's projection conv
    and conv1 both read stage 0's output, which the decoder reads too (three consumers of one tensor, no pool in
    between).  Every gradient upstream of that tensor (stem, stage 0) depends on all three contributions arriving."""
    strides = [[1, 1, 1], [1, 1, 1], [2, 2, 2]]
    ref_net = resenc_ref.build(strides=strides, zero_init=False)
    sd = {k: v.clone() for k, v in ref_net.state_dict().items()}
    b = resenc_ref.batch(strides=strides)
    r = resenc_ref.forward_backward(ref_net, b, torch.float64)
    net = _hip_net(sd, strides=strides)
    blk = net.encoder.stages[1].blocks[0]
    assert blk._proj and not blk._pool
    _check_fwd_bwd(net, _gbatch(b), r)


def test_network_2d_twin_matches_the_fp64_restatement():
    from oracle import step_oracle as SO
    st3 = [[1, 1, 1], [1, 2, 2], [1, 2, 2]]
    ref_net = resenc_ref.build(strides=st3, kernel_sizes=[[1, 3, 3]] * 3, zero_init=False)
    sd = resenc_ref.to2d_state_dict({k: v.clone() for k, v in ref_net.state_dict().items()})
    b2 = SO.synthetic_batch(resenc_ref.BATCH, resenc_ref.IN_CH, (16, 16), [[1, 1], [2, 2], [2, 2]],
                            num_classes=resenc_ref.CLASSES, seed=resenc_ref.BATCH_SEED)
    b3 = {'data': b2['data'].unsqueeze(2), 'target': [t.unsqueeze(2) for t in b2['target']]}
    r = resenc_ref.forward_backward(ref_net, b3, torch.float64)
    net = _hip_net(sd, nn.Conv2d, [[1, 1], [2, 2], [2, 2]])
    _check_fwd_bwd(net, _gbatch(b2), r, squeeze=True)


# ================================================================================================ trainer
def _trainer(graph=None, sd=None, cls="nnUNetTrainerMI355"):
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(resenc_ref.PATCH, resenc_ref.STRIDES, batch_size=resenc_ref.BATCH,
                               unet_class_name='ResidualEncoderUNet', n_blocks_per_stage=resenc_ref.BLOCKS,
                               n_conv_per_stage_decoder=(1, 1))
    tr = getattr(trainer, cls)(plans, "3d_fullres", 0, resenc_ref.DATASET_JSON, device=DEV)
    if graph is not None:
        tr.use_hip_graph = graph
    torch.manual_seed(0)
    tr.initialize()
    tr.network.load_state_dict(resenc_ref.reference64()['sd0'] if sd is None else sd, strict=True)
    tr.optimizer.fp.invalidate_packs()
    tr.on_train_epoch_start()
    return tr


def test_trainer_steps_match_the_stepped_oracle():
    from multimodal_mvd_seg_amd import network
    r = resenc_ref.reference64()
    tr = _trainer()
    assert isinstance(tr.network, network.MI355ResidualEncoderUNet)
    gb = _gbatch(resenc_ref.batch())
    for step in (1, 2, 3):
        res = tr.train_step(gb)
        ref_l = r['losses'][step - 1]
        assert abs(float(res["loss"]) - ref_l) <= 1e-5 * max(1.0, abs(ref_l)), (step, float(res["loss"]), ref_l)
        if step in (1, 3):
            for n, p in tr.network.named_parameters():
                close(p, r['params'][step][n], 1e-5, 0, f"param after step {step}: {n}")


def test_graphed_step_is_bit_identical_to_eager_with_validation_and_inference_in_between():
    from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor
    a = _trainer(graph=False)      # eager, never validates
    b = _trainer(graph=True)       # hip_graph_warmup eager steps, capture, replays; validates in between
    assert b.hip_graph_warmup == 3
    batches = [_gbatch(resenc_ref.batch(100 + i)) for i in range(8)]
    la, lb = [], []
    for i, bt in enumerate(batches):
        la.append(np.asarray(a.train_step(bt)["loss"]).copy())
        lb.append(np.asarray(b.train_step(bt)["loss"]).copy())
        if i == 5:       # 3 eager + the capture + 2 replays done; 2 more replays follow
            assert b._step_graph is not None and b._step_graph["graph"] is not None, "the step was never captured"
            b.validation_step(batches[0])
            img = torch.randn(resenc_ref.IN_CH, 14, 20, 16, generator=torch.Generator().manual_seed(9))
            SlidingWindowPredictor(b.network, resenc_ref.PATCH, resenc_ref.CLASSES, 0.5, True, True, (0, 1, 2),
                                   DEV).predict_sliding_window_return_logits(img)
            torch.cuda.synchronize()
            assert b.network.training and b.network.decoder.deep_supervision
    torch.cuda.synchronize()
    assert a._step_graph is None
    for i, (x, y) in enumerate(zip(la, lb)):
        assert np.array_equal(x, y), f"loss of step {i}: eager {x} graph {y}"
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def test_checkpoint_round_trip_keeps_keys_and_the_next_step():
    a = _trainer(graph=False)
    gb = _gbatch(resenc_ref.batch())
    a.train_step(gb)
    f = io.BytesIO()
    torch.save({"network_weights": a.network.state_dict(), "optimizer_state": a.optimizer.state_dict()}, f)
    f.seek(0)
    ck = torch.load(f, map_location="cpu", weights_only=False)
    assert list(ck["network_weights"].keys()) == list(resenc_ref.build().state_dict().keys())
    resenc_ref.build().load_state_dict(ck["network_weights"], strict=True)      # a torch restatement reads the checkpoint
    b = _trainer(graph=False, sd=ck["network_weights"])
    b.optimizer.load_state_dict({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ck["optimizer_state"].items()})
    la, lb = a.train_step(gb)["loss"], b.train_step(gb)["loss"]
    assert np.array_equal(np.asarray(la), np.asarray(lb)), (la, lb)
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def test_sliding_window_predictor_vs_the_fp64_restatement():
    from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor
    from oracle import infer_oracle as IO
    ora = resenc_ref.build(deep_supervision=False, zero_init=False)
    sd = {k: v.clone() for k, v in ora.state_dict().items()}
    ora = ora.double().eval()
    net = _hip_net(sd)
    img = torch.randn(resenc_ref.IN_CH, 24, 20, 20, generator=torch.Generator().manual_seed(5))
    pred = SlidingWindowPredictor(net, resenc_ref.PATCH, resenc_ref.CLASSES, 0.5, True, True, (0, 1, 2), DEV)
    out = pred.predict_sliding_window_return_logits(img)
    assert net.training and net.decoder.deep_supervision is True     # restored

    def oracle_net(x):
        with torch.no_grad():
            return ora(x.double()).float()

    ref = IO.predict_sliding_window_return_logits(oracle_net, img, resenc_ref.PATCH, resenc_ref.CLASSES, 0.5, True, (0, 1, 2))
    close(out, ref, 2e-5, 1e-5, "sliding-window logits")
