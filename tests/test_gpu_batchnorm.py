"""GPU tests of the BatchNorm3d path (nnUNetTrainerBN.py:31-32): the fused BatchNorm3d + LeakyReLU kernels against
torch.nn.functional.batch_norm in fp64 (the reference's BN IS torch.nn.BatchNorm3d), the BN network and trainer against the
oracle network with its norms swapped (tests/bn_ref.py), the graphed step against the eager step, and eval mode through the
sliding-window predictor.

Bars (the project's own from the InstanceNorm tests): y 2e-6 absolute and relative, dx 5e-6 x max, dgamma / dbeta 1e-5 x max,
running buffers 2e-6 relative (the kernel rounds them once from fp64); bf16 storage: the close_bf16 / close_f32 rules of
tests/test_gpu_bf16.py, restated here.

Every input carries a per-sample offset (sample n shifted by 1.5 n): per-sample and per-batch statistics then differ by far
more than any bar, so a kernel that normalises per sample cannot pass."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CL = torch.channels_last_3d


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


def close_bf16(a, ref, what):      # tests/test_gpu_bf16.py: 1 bf16 ulp (2^-8 relative, written 2^-7) + 2e-3 of the scale
    a, ref = a.float().cpu().double(), ref.double()
    tol = 2.0 ** -7 * ref.abs() + 2e-3 * float(ref.abs().max())
    err = (a - ref).abs()
    assert bool((err <= tol).all()), f"{what}: max err {float(err.max()):.3e} at |ref| {float(ref.abs().max()):.3e}"


def close_f32(a, ref, what, rel=2e-5):   # tests/test_gpu_bf16.py
    a, ref = a.float().cpu().double(), ref.double()
    err = float((a - ref).abs().max())
    assert err <= rel * float(ref.abs().max()) + 1e-7, f"{what}: max err {err:.3e} at |ref| {float(ref.abs().max()):.3e}"


def _inputs(N, C, sp, seed, xb=False, gyb=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, *sp, generator=g) * 0.7 + 0.2 + 1.5 * torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1, 1)
    gy = torch.randn(N, C, *sp, generator=g)
    if xb:
        x = x.to(torch.bfloat16)
    if gyb:
        gy = gy.to(torch.bfloat16)
    return dict(x=x, gy=gy, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.1,
                rm=torch.randn(C, generator=g) * 0.3, rv=torch.rand(C, generator=g) + 0.5)


def _reference(t, training, momentum):
    """F.leaky_relu(F.batch_norm(...)) in fp64 with autograd; the fp64 running buffers are updated in place."""
    xr, gr, br = (t[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    rm, rv = t["rm"].double().clone(), t["rv"].double().clone()
    ref = F.leaky_relu(F.batch_norm(xr, rm, rv, gr, br, training, momentum, 1e-5), 0.01)
    if training:
        ref.backward(t["gy"].double())
    return ref.detach(), xr.grad, gr.grad, br.grad, rm, rv


def _hip(t, training, momentum, nbt, out_bf16=False):
    from multimodal_mvd_seg_amd import ops
    gx = t["x"].to(DEV).contiguous(memory_format=CL).requires_grad_()
    gg, gb = t["gamma"].to(DEV).requires_grad_(), t["beta"].to(DEV).requires_grad_()
    rm, rv = t["rm"].to(DEV), t["rv"].to(DEV)
    y = ops.BatchNormLeakyReLUFn.apply(gx, gg, gb, rm, rv, nbt, 1e-5, momentum, 0.01, training, out_bf16)
    if training:
        y.backward(t["gy"].to(DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    return y.detach(), gx.grad, gg.grad, gb.grad, rm, rv, gx


def _buffers_close(a, ref64, what):
    """fp32 values rounded once from fp64: every entry within 2e-6 of itself."""
    a, r = a.cpu().double(), ref64.float().double()
    rel = float(((a - r).abs() / r.abs()).max())
    print(f"{what}: max relative err {rel:.3e}")
    assert rel <= 2e-6, f"{what}: max relative err {rel:.3e}"


BIG = (3, 32, (48, 48, 48))   # 216 blocks per sample: a channel's finalize sums 648 partials, more than a wave has lanes
SHAPES = [(3, 5, (3, 3, 3)),         # C % 4 != 0, odd V
          (2, 320, (2, 2, 2)),       # many channels, few voxels
          (1, 32, (8, 8, 8)),        # N = 1
          (2, 64, (6, 5, 7)),
          BIG]


@pytest.mark.parametrize("momentum", [0.1, 0.3])
@pytest.mark.parametrize("N,C,sp", SHAPES)
def test_training_forward_backward_and_running_buffers_vs_fp64(N, C, sp, momentum):
    from multimodal_mvd_seg_amd._lib import query
    V = sp[0] * sp[1] * sp[2]
    nblk = query("mvd_batchnorm_nblk", N, V, C)
    assert nblk >= 1
    if (N, C, sp) == BIG:
        assert N * nblk > 64 and nblk > 64, f"{N} x {nblk} block partials per channel: the finalize loop is not exercised"
    t = _inputs(N, C, sp, seed=N * 1000 + C + int(momentum * 10))
    ref, dx_r, dg_r, db_r, rm_r, rv_r = _reference(t, True, momentum)
    # the per-sample statistics are far from the batch statistics (guards against an InstanceNorm in disguise)
    if N > 1:
        inst = F.leaky_relu(F.instance_norm(t["x"].double(), None, None, t["gamma"].double(), t["beta"].double(), True, 0.1,
                                            1e-5), 0.01)
        assert float((inst - ref).abs().max()) > 0.1
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y, dx, dg, db, rm, rv, _ = _hip(t, True, momentum, nbt)
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=CL) and dx.dtype == torch.float32
    close(y, ref, 2e-6, 2e-6, "y")
    close(dx, dx_r, 5e-6 * float(dx_r.abs().max()), 0, "dx")
    close(dg, dg_r, 1e-5 * float(dg_r.abs().max()), 0, "dgamma")
    close(db, db_r, 1e-5 * float(db_r.abs().max()), 0, "dbeta")
    _buffers_close(rm, rm_r, "running_mean")
    _buffers_close(rv, rv_r, "running_var")     # (unbiased: M / (M - 1), as torch)
    M = N * V
    var_b = t["x"].double().transpose(0, 1).reshape(C, -1).var(1, unbiased=False)
    exp_rv = (1 - momentum) * t["rv"].double() + momentum * var_b * M / (M - 1)
    assert float(((rv_r - exp_rv).abs() / exp_rv).max()) < 1e-12   # (the oracle itself applies the unbiased factor)
    assert int(nbt) == 1
    # the same call again: bit-equal (fixed-order sums, no atomics); the counter moves on
    y2, dx2, dg2, db2, rm2, rv2, _ = _hip(t, True, momentum, nbt)
    assert int(nbt) == 2
    for a, b, what in ((y, y2, "y"), (dx, dx2, "dx"), (dg, dg2, "dgamma"), (db, db2, "dbeta"), (rm, rm2, "running_mean"),
                       (rv, rv2, "running_var")):
        assert torch.equal(a, b), f"{what}: two identical calls differ"


def test_one_value_per_channel_is_refused_on_the_device_too():
    t = _inputs(1, 8, (1, 1, 1), seed=1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _hip(t, True, 0.1, torch.zeros((), dtype=torch.int64, device=DEV))
    from multimodal_mvd_seg_amd._lib import load
    import ctypes
    lib = load()
    x = torch.zeros(8, device=DEV)
    P = lambda v: ctypes.c_void_p(v.data_ptr())      # noqa: E731
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    rc = lib.mvd_batchnorm_lrelu_fwd(P(x), 0, P(x), P(x), P(x), 0, P(x), P(x), P(x), P(x), P(nbt), 1, 1, 8, 1e-5, 0.1, 0.01,
                                     P(ws), ws.numel(), None)
    assert rc == 2 and b"more than 1 value per channel" in lib.mvd_last_error()
    assert int(nbt) == 0


@pytest.mark.parametrize("N,C,sp", [(3, 5, (3, 3, 3)), (2, 64, (6, 5, 7))])
def test_eval_forward_reads_the_running_buffers_and_leaves_them(N, C, sp):
    t = _inputs(N, C, sp, seed=77 + C)
    ref = _reference(t, False, 0.1)[0]
    batch_ref = _reference(t, True, 0.1)[0]
    assert float((ref - batch_ref).abs().max()) > 0.1          # running and batch statistics are far apart
    nbt = torch.full((), 5, dtype=torch.int64, device=DEV)
    y, _dx, _dg, _db, rm, rv, gx = _hip(t, False, 0.1, nbt)
    close(y, ref, 2e-6, 2e-6, "y (eval)")
    assert torch.equal(rm.cpu(), t["rm"]) and torch.equal(rv.cpu(), t["rv"]) and int(nbt) == 5
    from multimodal_mvd_seg_amd import ops
    y = ops.BatchNormLeakyReLUFn.apply(gx, t["gamma"].to(DEV), t["beta"].to(DEV), rm, rv, nbt, 1e-5, 0.1, 0.01, False)
    with pytest.raises(RuntimeError, match="backward through an eval-mode forward"):
        y.sum().backward()


@pytest.mark.parametrize("xb", [False, True])
@pytest.mark.parametrize("N,C,sp", [(2, 32, (8, 8, 8)), (1, 64, (6, 5, 7)), (2, 320, (2, 2, 2))])
def test_bf16_io(N, C, sp, xb):
    """fp32-or-bf16 conv output -> bf16 activation; statistics and arithmetic as the fp32 kernel, so against fp64 on the same
    (rounded) operands the output is 1 bf16 ulp, dgamma / dbeta and the running buffers are fp32-accurate; dx has x's dtype."""
    t = _inputs(N, C, sp, seed=N * C + int(xb), xb=xb, gyb=True)
    ref, dx_r, dg_r, db_r, rm_r, rv_r = _reference(t, True, 0.1)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y, dx, dg, db, rm, rv, _ = _hip(t, True, 0.1, nbt, out_bf16=True)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL) and dx.dtype == t["x"].dtype
    close_bf16(y, ref, "y")
    (close_bf16 if xb else close_f32)(dx, dx_r, "dx")
    close_f32(dg, dg_r, "dgamma")
    close_f32(db, db_r, "dbeta")
    _buffers_close(rm, rm_r, "running_mean")
    _buffers_close(rv, rv_r, "running_var")
    assert int(nbt) == 1
    # eval with bf16 storage
    nbt5 = torch.full((), 5, dtype=torch.int64, device=DEV)
    ye = _hip(t, False, 0.1, nbt5, out_bf16=True)[0]
    assert ye.dtype == torch.bfloat16
    close_bf16(ye, _reference(t, False, 0.1)[0], "y (eval)")


# ================================================================================================ network and trainer
def _trainer(precision="fp32", graph=None, sd=None):
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(bn_ref.PATCH, bn_ref.STRIDES, batch_size=bn_ref.BATCH)
    tr = trainer.nnUNetTrainerBNMI355(plans, "3d_fullres", 0, bn_ref.DATASET_JSON, device=DEV)
    tr.precision = precision
    if graph is not None:
        tr.use_hip_graph = graph
    torch.manual_seed(0)
    tr.initialize()
    tr.network.load_state_dict(bn_ref.reference64()['sd0'] if sd is None else sd, strict=True)
    tr.optimizer.fp.invalidate_packs()
    tr.on_train_epoch_start()
    return tr


def _gbatch(seed=bn_ref.BATCH_SEED):
    b = bn_ref.batch(seed)
    return {"data": b["data"].to(DEV), "target": [t.to(DEV) for t in b["target"]]}


def _check_buffers(net, ref, what):
    got = dict(net.named_buffers())
    assert set(got) == set(ref)
    for n, v in ref.items():
        if v.dtype.is_floating_point:
            close(got[n], v, bn_ref.buffer_tol(v), 0, f"{what}: {n}")
        else:
            assert int(got[n]) == int(v), f"{what}: {n} = {int(got[n])}, expected {int(v)}"


def test_bn_network_training_mode_matches_the_swapped_oracle_in_fp64():
    from multimodal_mvd_seg_amd import network
    r = bn_ref.reference64()
    tr = _trainer()
    assert all(isinstance(b.norm, network.HipBatchNorm3d) for b in tr.network.modules()
               if isinstance(b, network.ConvDropoutNormReLU))
    # interchange, the other direction: our state_dict loads into the swapped oracle, strictly
    bn_ref.bn_oracle().load_state_dict({k: v.cpu() for k, v in tr.network.state_dict().items()}, strict=True)
    gb = _gbatch()
    assert tr.network.training
    tr.optimizer.zero_grad()
    out = tr.network(gb["data"])
    l = tr.loss(out, gb["target"])
    l.backward()
    for i, (o, ref) in enumerate(zip(out, r['logits'])):
        assert o.dtype == torch.float32 and o.is_contiguous()
        close(o, ref, 1e-4, 0, f"logits{i}")
    assert abs(float(l) - r['losses'][0]) <= 1e-5 * max(1.0, abs(r['losses'][0])), (float(l), r['losses'][0])
    for n, p in tr.network.named_parameters():
        close(p.grad, r['grads'][n], bn_ref.grad_tol(n, r['grads'][n]), 0, "grad " + n)
    _check_buffers(tr.network, r['buffers'][1], "buffers after one training forward")


def test_bn_trainer_steps_match_the_stepped_oracle():
    r = bn_ref.reference64()
    tr = _trainer()
    gb = _gbatch()
    for step in (1, 2, 3):
        res = tr.train_step(gb)
        ref_l = r['losses'][step - 1]
        assert abs(float(res["loss"]) - ref_l) <= 1e-5 * max(1.0, abs(ref_l)), (step, float(res["loss"]), ref_l)
        if step in (1, 3):
            for n, p in tr.network.named_parameters():
                close(p, r['params'][step][n], 1e-5, 0, f"param after step {step}: {n}")
            _check_buffers(tr.network, r['buffers'][step], f"buffers after step {step}")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_bn_step_is_bit_identical_to_eager_with_validation_and_inference_in_between(precision):
    from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor
    a = _trainer(precision, graph=False)      # eager, never validates
    b = _trainer(precision, graph=True)       # hip_graph_warmup eager steps, capture, replays; validates in between
    assert b.hip_graph_warmup == 3
    batches = [_gbatch(100 + i) for i in range(8)]
    la, lb = [], []
    for i, bt in enumerate(batches):
        la.append(np.asarray(a.train_step(bt)["loss"]).copy())
        lb.append(np.asarray(b.train_step(bt)["loss"]).copy())
        if i == 5:       # 3 eager + the capture + 2 replays done; 2 more replays follow
            assert b._step_graph is not None and b._step_graph["graph"] is not None, "the step was never captured"
            before = {n: v.clone() for n, v in b.network.named_buffers()}
            b.validation_step(batches[0])
            img = torch.randn(bn_ref.IN_CH, 14, 20, 16, generator=torch.Generator().manual_seed(9))
            SlidingWindowPredictor(b.network, bn_ref.PATCH, bn_ref.CLASSES, 0.5, True, True, (0, 1, 2),
                                   DEV).predict_sliding_window_return_logits(img)
            torch.cuda.synchronize()
            assert b.network.training and b.network.decoder.deep_supervision
            for n, v in b.network.named_buffers():
                assert torch.equal(v, before[n]), f"{n} changed during validation / inference"
    torch.cuda.synchronize()
    assert a._step_graph is None
    for i, (x, y) in enumerate(zip(la, lb)):
        assert np.array_equal(x, y), f"loss of step {i}: eager {x} graph {y}"
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    bufs_b = dict(b.network.named_buffers())
    for n, v in a.network.named_buffers():
        assert torch.equal(v, bufs_b[n]), n
        if n.endswith("num_batches_tracked"):
            assert int(v) == len(batches), (n, int(v))


def test_eval_through_the_sliding_window_predictor_uses_the_running_statistics():
    from multimodal_mvd_seg_amd import network
    from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor
    from oracle import infer_oracle as IO
    ora, sd = bn_ref.eval_oracle(deep_supervision=False)
    net = network.MI355PlainConvUNet(bn_ref.IN_CH, 3, bn_ref.FEATURES, nn.Conv3d, 3, bn_ref.STRIDES, 2, bn_ref.CLASSES, 2, True,
                                     nn.BatchNorm3d, {'eps': 1e-5, 'affine': True}, None, None, nn.LeakyReLU,
                                     {'inplace': True}, deep_supervision=True)
    net.load_state_dict(sd, strict=True)
    net.to(DEV)
    assert all(b.is_cuda for b in net.buffers())
    img = torch.randn(bn_ref.IN_CH, 14, 22, 25, generator=torch.Generator().manual_seed(5))
    pred = SlidingWindowPredictor(net, bn_ref.PATCH, bn_ref.CLASSES, 0.5, True, True, (0, 1, 2), DEV)
    out = pred.predict_sliding_window_return_logits(img)
    assert net.training and net.decoder.deep_supervision is True     # restored
    for n, v in net.state_dict().items():
        assert torch.equal(v.cpu(), sd[n]), f"{n} changed during inference"

    def oracle_net(x):
        with torch.no_grad():
            return ora(x.double()).float()

    ref = IO.predict_sliding_window_return_logits(oracle_net, img, bn_ref.PATCH, bn_ref.CLASSES, 0.5, True, (0, 1, 2))
    close(out, ref, 2e-5, 1e-5, "sliding-window logits")
    # eval is not the training-mode forward in disguise
    x = torch.randn(2, bn_ref.IN_CH, *bn_ref.PATCH, generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        net.eval()
        ye = net(x)[0]
        net.train()
        yt = net(x)[0]
    assert float((ye - yt).abs().max()) > 1e-2


def test_bn_network_bf16_step():
    """One train step in bf16 mixed precision: fp32 logits, and the loss inside the band tests/test_gpu_bf16.py holds the
    InstanceNorm network to -- no further from the fp64 evaluation than twice torch's own CPU autocast(bf16) evaluation of
    the same network, or 2e-3 of the loss."""
    from oracle import loss_oracle as LO
    r = bn_ref.reference64()
    l64 = r['losses'][0]
    cb = bn_ref.batch()
    oac = bn_ref.bn_oracle()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        l_ac = LO.build_loss(len(cb['target']))(oac(cb['data']), cb['target'])
    tr = _trainer("bf16")
    gb = _gbatch()
    with torch.no_grad():
        out = tr.network(gb["data"])
        l = tr.loss(out, gb["target"])
    assert all(o.dtype == torch.float32 for o in out)
    band = max(2 * abs(float(l_ac) - l64), 2e-3 * abs(l64))
    print(f"bf16 loss {float(l):.6f} fp64 {l64:.6f} autocast {float(l_ac):.6f} band {band:.3e}")
    assert abs(float(l) - l64) <= band
    bufs = dict(tr.network.named_buffers())
    assert all(v.dtype == torch.float32 for n, v in bufs.items() if "running_" in n)
    res = tr.train_step(gb)
    assert np.isfinite(float(res["loss"]))
    assert all(int(v) == 2 for n, v in tr.network.named_buffers() if n.endswith("num_batches_tracked"))
