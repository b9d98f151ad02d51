"""GPU tests of the plain loss kernels (csrc/loss.hip: k_dcce_*, k_argmax_counts, k_softmax_select, k_label_mask, k_kl,
k_kl_rows, k_mse_*; csrc/topo.hip: k_dot_sum, k_cldice_combine) against oracle/loss_oracle.py evaluated in float64 on
the CPU (tests/losses_ref.py), at the shapes the fixture tests of test_gpu_parity.py do not reach: every K / C, voxel
counts that are no multiple of 4 or 256, the grid-stride loops, strided and misaligned operands, one-sided gradients.
Bars are the project's: loss 1e-5 relative, every gradient / element-wise output 1e-5 * max|reference|,
integers bit-exact.  Every device evaluation runs twice and must repeat bit for bit (fixed-order reductions)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import losses_ref as LR
from multimodal_mvd_seg_amd import losses, ops
from multimodal_mvd_seg_amd._lib import call, query

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
LOSS_TOL, GRAD_TOL = 1e-5, 1e-5
CL3D = torch.channels_last_3d
SMALL = (5, 7, 9)        # V = 315: no multiple of 4 or 256, two blocks of 256
BIG = (41, 41, 41)       # V = 68 921 (odd): with N from the launch caps below the grid-stride loops run twice and more


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


# ------------------------------------------------------------------------------------------------ helpers
def labels(g, N, K, shape, absent=()):
    """float label map [N,1,*shape] over the classes 0..K-1 without `absent`"""
    pool = torch.tensor([k for k in range(K) if k not in absent], dtype=torch.float32)
    return pool[torch.randint(0, len(pool), (N, 1, *shape), generator=g)]


@functools.lru_cache(maxsize=None)
def big_logits(N, K):
    """[N,K,41^3] logits and labels, generated once and shared (never written to)"""
    g = torch.Generator().manual_seed(1000 + 10 * N + K)
    return torch.randn((N, K, *BIG), generator=g) * 2.0, labels(g, N, K, BIG)


def twice(fn):
    """run a device evaluation twice: (loss, [grads]) on the host, bit-identical between the runs"""
    a, b = fn(), fn()
    assert torch.equal(a[0], b[0]), "loss differs between two runs"
    for x, y in zip(a[1], b[1]):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), "gradient differs between two runs"
    return a


def dev_loss(loss_fn, inputs, need=None, scale=None):
    """loss_fn(*device leaves) -> backward -> (loss, [grad or None]); inputs keep their strides on the way to the device"""
    need = [True] * len(inputs) if need is None else need

    def run():
        leaves = [t.to(DEV).requires_grad_(n) for t, n in zip(inputs, need)]
        l = loss_fn(*leaves)
        (l if scale is None else l * scale).backward()
        torch.cuda.synchronize()
        return l.detach().cpu(), [None if t.grad is None else t.grad.cpu() for t in leaves]
    return twice(run)


def check(got, want, what):
    (l, g), (lr, gr) = got, want
    lerr = abs(float(l) - float(lr)) / max(abs(float(lr)), 1e-300)
    msg = f"{what}: loss {float(l):.8f} ref {float(lr):.8f} rel {lerr:.2e};"
    assert len(g) == len(gr)
    worst = []
    for a, b in zip(g, gr):
        assert (a is None) == (b is None), f"{what}: gradient present on one side only"
        if a is None:
            continue
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), what
        gmax, gerr = float(b.abs().max()), float((a.double() - b).abs().max())
        msg += f" grad err {gerr:.2e} of max|g| {gmax:.2e} ({gerr / max(gmax, 1e-300):.2e});"
        worst.append((gerr, gmax))
    print(msg)
    assert np.isfinite(float(l))
    assert lerr <= LOSS_TOL, lerr
    for gerr, gmax in worst:
        assert gerr <= GRAD_TOL * gmax, (gerr, gmax)


def check_elementwise(got, want, what):
    err, m = float((got.double() - want).abs().max()), float(want.abs().max())
    print(f"{what}: err {err:.2e} of max {m:.2e} ({err / max(m, 1e-300):.2e})")
    assert bool(torch.isfinite(got).all()) and err <= GRAD_TOL * m, (err, m)


def dcce(batch_dice, do_bg, smooth, w_ce=1, w_dice=1):
    return losses.DC_and_CE_loss({'batch_dice': batch_dice, 'smooth': smooth, 'do_bg': do_bg, 'ddp': False}, {},
                                 weight_ce=w_ce, weight_dice=w_dice)


def ndhwc(t):
    return t.contiguous(memory_format=CL3D)


def misaligned(t):
    """the same values as a dense view one float into a larger device buffer: not 16-byte aligned"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].as_strided(t.shape, t.stride())
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.stride() == t.stride()
    return v


# ================================================================================================ 1. DC + CE
@pytest.mark.parametrize("do_bg", [False, True])
@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_dcce_matrix(K, N, batch_dice, do_bg):
    g = torch.Generator().manual_seed(100 * K + 10 * N + 2 * batch_dice + do_bg)
    z, t = torch.randn((N, K, *SMALL), generator=g) * 3.0, labels(g, N, K, SMALL)
    tag = f"K={K} N={N} batch_dice={batch_dice} do_bg={do_bg}"
    for smooth, w_ce, w_dice in ((1e-5, 1, 1), (1.0, 1, 1), (1e-5, 0.3, 1.7), (1.0, 0.3, 1.7)):
        check(dev_loss(lambda x: dcce(batch_dice, do_bg, smooth, w_ce, w_dice)(x, t.to(DEV)), [z]),
              LR.dc_ce(z, t, batch_dice, do_bg, smooth, w_ce, w_dice), f"{tag} smooth={smooth} w=({w_ce},{w_dice})")
    check(dev_loss(lambda x: losses.RobustCrossEntropyLoss()(x, t.to(DEV)), [z]), LR.ce_only(z, t), f"{tag} CE only")
    # Dice alone, smooth / ddp from its own constructor defaults (1.0, True: no process group, so no gather)
    check(dev_loss(lambda x: losses.MemoryEfficientSoftDiceLoss(batch_dice=batch_dice, do_bg=do_bg)(x, t.to(DEV)), [z]),
          LR.dice_only(z, t, batch_dice=batch_dice, do_bg=do_bg), f"{tag} Dice only")
    if not batch_dice and do_bg:     # these two ARE the constructor defaults
        check(dev_loss(lambda x: losses.MemoryEfficientSoftDiceLoss()(x, t.to(DEV)), [z]), LR.dice_only(z, t),
              f"{tag} Dice only, all defaults")


def test_dcce_upstream_gradient_scale():
    """(loss * 2.5).backward(): the upstream gradient reaches k_dcce_bwd through gscale_dev"""
    g = torch.Generator().manual_seed(7)
    z, t = torch.randn((2, 5, *SMALL), generator=g) * 3.0, labels(g, 2, 5, SMALL)
    for bd in (False, True):
        got = dev_loss(lambda x: dcce(bd, False, 1e-5)(x, t.to(DEV)), [z], scale=2.5)
        check(got, LR.dc_ce(z, t, bd, False, 1e-5, scale=2.5), f"upstream 2.5 batch_dice={bd}")
        plain = LR.dc_ce(z, t, bd, False, 1e-5)
        check(got, (plain[0], [2.5 * plain[1][0]]), f"2.5 x the plain gradient batch_dice={bd}")


@pytest.mark.parametrize("batch_dice,do_bg", [(True, False), (False, True)])
def test_dcce_grid_stride_loops(batch_dice, do_bg):
    # mvd_dcce_fwd: cap_per_n(2048, N) = 128 blocks per sample at N = 16, mvd_dcce_bwd: cap_per_n(4096, N) = 256;
    # V = 68 921 is 270 blocks of 256 (the last one 57 voxels): both loops take a second, ragged trip
    z, t = big_logits(16, 8)
    check(dev_loss(lambda x: dcce(batch_dice, do_bg, 1e-5)(x, t.to(DEV)), [z]), LR.dc_ce(z, t, batch_dice, do_bg, 1e-5),
          f"[16,8,41^3] batch_dice={batch_dice} do_bg={do_bg}")


@pytest.mark.parametrize("batch_dice", [False, True])
def test_dcce_absent_classes(batch_dice):
    g = torch.Generator().manual_seed(11)
    z = torch.randn((3, 5, *SMALL), generator=g) * 3.0
    t = labels(g, 3, 5, SMALL)
    t[1] = labels(g, 1, 5, SMALL, absent=(2,))[0]          # class 2 missing from sample 1 only
    assert bool((t[1] != 2).all()) and bool((t[0] == 2).any())
    check(dev_loss(lambda x: dcce(batch_dice, False, 1e-5)(x, t.to(DEV)), [z]), LR.dc_ce(z, t, batch_dice, False, 1e-5),
          f"class absent from one sample, batch_dice={batch_dice}")
    t = labels(g, 3, 5, SMALL, absent=(3,))                # class 3 missing from the whole batch
    for do_bg in (False, True):
        check(dev_loss(lambda x: dcce(batch_dice, do_bg, 1e-5)(x, t.to(DEV)), [z]),
              LR.dc_ce(z, t, batch_dice, do_bg, 1e-5), f"class absent from the batch, batch_dice={batch_dice} do_bg={do_bg}")


@pytest.mark.parametrize("batch_dice", [False, True])
def test_dcce_denominator_clip(batch_dice):
    """smooth = 0, no voxel of class 4 and its probability underflowing everywhere: G + P + smooth < 1e-8 is clipped
    (torch.clip: value 1e-8, zero gradient through the clipped operand) -- in fp64 as on the device"""
    g = torch.Generator().manual_seed(13)
    z = torch.randn((2, 5, *SMALL), generator=g) * 3.0
    z[:, 4] = -200.0
    t = labels(g, 2, 5, SMALL, absent=(4,))
    got = dev_loss(lambda x: dcce(batch_dice, False, 0.0)(x, t.to(DEV)), [z])
    check(got, LR.dc_ce(z, t, batch_dice, False, 0.0), f"clip branch batch_dice={batch_dice}")


def test_dcce_large_logits():
    g = torch.Generator().manual_seed(17)
    z, t = torch.randn((2, 5, *SMALL), generator=g) * 40.0, labels(g, 2, 5, SMALL)
    for bd in (False, True):
        check(dev_loss(lambda x: dcce(bd, False, 1e-5)(x, t.to(DEV)), [z]), LR.dc_ce(z, t, bd, False, 1e-5),
              f"logits x 40 batch_dice={bd}")


def test_dcce_label_map_forms():
    """float labels as [N,1,...] and as [N,...]: the same loss and gradient bit for bit, and the oracle's"""
    g = torch.Generator().manual_seed(19)
    z, t = torch.randn((2, 5, *SMALL), generator=g) * 3.0, labels(g, 2, 5, SMALL)
    a = dev_loss(lambda x: dcce(True, False, 1e-5)(x, t.to(DEV)), [z])
    b = dev_loss(lambda x: dcce(True, False, 1e-5)(x, t[:, 0].to(DEV)), [z])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    check(b, LR.dc_ce(z, t, True, False, 1e-5), "labels as [N,...]")


def test_dcce_deep_supervision():
    g = torch.Generator().manual_seed(23)
    shapes = [(8, 10, 12), (4, 5, 6), (2, 3, 3)]
    zs = [torch.randn((2, 5, *s), generator=g) * 3.0 for s in shapes]
    ts = [labels(g, 2, 5, s) for s in shapes]
    w = losses.ds_weights(3)
    assert w[-1] == 0 and w[0] > 0 and w[1] > 0
    for bd in (False, True):
        wrapper = losses.DeepSupervisionWrapper(dcce(bd, False, 1e-5), w)
        got = dev_loss(lambda *x: wrapper(list(x), [t.to(DEV) for t in ts]), zs)
        assert got[1][-1].shape == zs[-1].shape and bool((got[1][-1] == 0).all())   # zero weight: exact zeros, not None
        check(got, LR.deep_supervised(zs, ts, [float(x) for x in w], bd, False, 1e-5), f"deep supervision batch_dice={bd}")


def device_stats(z, t):
    """per-sample (I, P, G) x K + CE sums of another batch, straight from mvd_dcce_fwd"""
    x = z.to(DEV).contiguous()
    N, K = x.shape[:2]
    V = x[0, 0].numel()
    tt = t.to(DEV).reshape(N, V).contiguous()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    stats = torch.empty((N, 3 * K + 1), device=DEV)
    ws = torch.empty(query("mvd_dcce_workspace_bytes", N, V, K), dtype=torch.uint8, device=DEV)
    call("mvd_dcce_fwd", p(x), p(tt), p(stats), N, V, K, p(ws), ws.numel(),
         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return stats


@pytest.mark.parametrize("do_bg", [False, True])
def test_dcce_ddp_batch_dice_slicing_single_process(do_bg):
    """DeepSupervisedDCCEFn with a stub `gather`: the Dice statistics of a second, different batch in front of the
    local ones (Nd = 5 != N = 2, off = 3) and a gradient multiplier of 2"""
    g = torch.Generator().manual_seed(29)
    z, t = torch.randn((2, 5, *SMALL), generator=g) * 3.0, labels(g, 2, 5, SMALL)
    zo, to = torch.randn((3, 5, *SMALL), generator=g) * 2.0 + 0.5, labels(g, 3, 5, SMALL, absent=(1,))
    stats_other = device_stats(zo, to)
    seen = []

    def gather(stats):
        seen.append(tuple(stats.shape))
        return torch.cat([stats_other, stats]), 3, 2.0
    w_ce, w_dice = 0.3, 1.7
    cfg = (True, do_bg, 1e-5, w_ce, w_dice)
    got = dev_loss(lambda x: ops.DeepSupervisedDCCEFn.apply([1.0], cfg, gather, [t.to(DEV)], x), [z])
    assert seen == [(2, 16), (2, 16)]
    want = LR.dc_ce_gathered(z, t, zo, to, do_bg, 1e-5, w_ce, w_dice, 2.0)
    check(got, want[:2], f"stub gather do_bg={do_bg}")


@pytest.mark.parametrize("K", [9, 1])
def test_dcce_refuses_class_counts_outside_2_to_8(K):
    z = torch.zeros((1, K, 4, 4, 4), device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="bad shape"):      # the host check of mvd_dcce_fwd, in front of any launch
        dcce(False, False, 1e-5)(z, torch.zeros((1, 1, 4, 4, 4), device=DEV))
    torch.cuda.synchronize()


# ================================================================================================ 2. argmax counts
def _check_counts(z, t):
    a = ops.argmax_counts(z.to(DEV), t.to(DEV)).cpu()
    b = ops.argmax_counts(z.to(DEV), t.to(DEV)).cpu()
    want = LR.argmax_counts(z, t)
    assert a.dtype == torch.int64 and torch.equal(a, b)
    assert int(want.sum()) > 0 and np.array_equal(a.numpy(), want), (a.numpy(), want)


@pytest.mark.parametrize("K", [2, 5, 8])
def test_argmax_counts_with_ties(K):
    g = torch.Generator().manual_seed(31 + K)
    z = torch.randint(-2, 3, (2, K, *SMALL), generator=g).float()      # integers in [-2, 2]: ties at most voxels
    assert float((z.max(1).values[:, None] == z).sum(1).float().mean()) > 1.1
    _check_counts(z, labels(g, 2, K, SMALL))


def test_argmax_counts_grid_stride_loop():
    # mvd_argmax_counts: cap_per_n(1024, N) = 64 blocks per sample at N = 16; V = 68 921 needs 270
    g = torch.Generator().manual_seed(37)
    z = torch.randint(-2, 3, (16, 8, *BIG), generator=g).float()
    _check_counts(z, big_logits(16, 8)[1])


# ================================================================================================ 3. softmax channel, label mask
def _softmax_select(z, gy, sels):
    zd = z.double().requires_grad_(True)
    p = torch.softmax(zd, 1)
    for sel in sels:
        def run():
            x = z.to(DEV).requires_grad_(True)
            y = ops.SoftmaxSelectFn.apply(x, sel)
            y.backward(gy.to(DEV))
            torch.cuda.synchronize()
            return y.detach().cpu(), [x.grad.cpu()]
        y, (gx,) = twice(run)
        want = p[:, sel:sel + 1]
        gref, = torch.autograd.grad(want, zd, gy.double(), retain_graph=True)
        assert y.shape == want.shape
        check_elementwise(y, want.detach(), f"softmax select K={z.shape[1]} sel={sel} fwd")
        check_elementwise(gx, gref, f"softmax select K={z.shape[1]} sel={sel} bwd")


@pytest.mark.parametrize("K", [2, 5, 8])
def test_softmax_select_every_channel(K):
    g = torch.Generator().manual_seed(41 + K)
    z, gy = torch.randn((2, K, *SMALL), generator=g) * 3.0, torch.randn((2, 1, *SMALL), generator=g)
    _softmax_select(z, gy, range(K))
    with pytest.raises(RuntimeError, match="bad arguments"):
        ops.SoftmaxSelectFn.apply(z.to(DEV), K)


@pytest.mark.parametrize("K", [2, 5, 8])
def test_softmax_select_grid_stride_loop(K):
    # mvd_softmax_select_fwd / _bwd: cap_per_n(4096, N) = 256 blocks per sample at N = 16; V = 68 921 needs 270
    z = big_logits(16, K)[0]
    gy = torch.randn((16, 1, *BIG), generator=torch.Generator().manual_seed(43))
    _softmax_select(z, gy, range(K))


@pytest.mark.parametrize("n", [315, 256 * 4096 + 4097])      # mvd_label_mask: at most 4096 blocks of 256; the second n is odd
def test_label_mask(n):
    g = torch.Generator().manual_seed(47)
    lab = labels(g, 1, 5, (n,), absent=(3,)).reshape(n)
    for v in (2, 3, 0):        # present, absent, background
        m = ops.label_mask(lab.to(DEV), v).cpu()
        want = (lab == v).float()
        assert (v == 3) == (not bool(want.any()))
        assert torch.equal(m, want) and torch.equal(m, ops.label_mask(lab.to(DEV), v).cpu())


# ================================================================================================ 4. KL
def _kl_pair(g, N, C, shape, scale=2.0):
    return torch.randn((N, C, *shape), generator=g) * scale, torch.randn((N, C, *shape), generator=g) * scale


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("C", [1, 2, 3, 7, 8, 31, 32])
def test_kl_generic_kernel_planar(C, T):
    ys, yt = _kl_pair(torch.Generator().manual_seed(50 + C), 2, C, SMALL)
    check(dev_loss(lambda a, b: losses.distill_kl(a, b, T), [ys, yt]), LR.kl(ys, yt, T), f"k_kl planar C={C} T={T}")
    if C > 1:      # the feature form (no epsilon, never padded) through the same kernel
        check(dev_loss(lambda a, b: losses.l2_loss(a, b, True, T), [ys, yt]), LR.kl(ys, yt, T, "l2"), f"k_kl l2 C={C} T={T}")


def test_kl_refuses_more_than_32_channels():
    ys, yt = _kl_pair(torch.Generator().manual_seed(53), 1, 33, (2, 3, 4))
    with pytest.raises(RuntimeError, match="C<=32"):
        losses.distill_kl(ys.to(DEV).requires_grad_(), yt.to(DEV))
    torch.cuda.synchronize()


def test_kl_generic_kernel_grid_stride_loop():
    # mvd_kl_fwd: at most 2048 blocks of 256 rows, mvd_kl_bwd (k_kl): 4096; [16,5,41^3] is 1 102 736 rows > 256 * 4096
    ys, yt = _kl_pair(torch.Generator().manual_seed(59), 16, 5, BIG)
    check(dev_loss(lambda a, b: losses.distill_kl(a, b, 2), [ys, yt]), LR.kl(ys, yt, 2), "k_kl [16,5,41^3] T=2")


@pytest.mark.parametrize("T", [1, 4])
def test_kl_strided_channel_slice(T):
    """x[:, 2:3] of planar [N,5,...] logits on both operands: the padded 1-channel branch with batch stride 5 V"""
    xs, xt = _kl_pair(torch.Generator().manual_seed(61), 2, 5, SMALL)

    def sliced(fn):
        def run():
            a, b = xs.to(DEV).requires_grad_(True), xt.to(DEV).requires_grad_(True)
            assert not a[:, 2:3].is_contiguous()
            l = fn(a, b)
            l.backward()
            torch.cuda.synchronize()
            return l.detach().cpu(), [a.grad.cpu(), b.grad.cpu()]
        return twice(run)
    got = sliced(lambda a, b: losses.distill_kl(a[:, 2:3], b[:, 2:3], T))
    for grad in got[1]:     # nothing flows into the other channels
        assert bool((grad[:, :2] == 0).all()) and bool((grad[:, 3:] == 0).all())
    dense = dev_loss(lambda a, b: losses.distill_kl(a, b, T), [xs[:, 2:3].contiguous(), xt[:, 2:3].contiguous()])
    assert torch.equal(got[0], dense[0])
    assert torch.equal(got[1][0][:, 2:3], dense[1][0]) and torch.equal(got[1][1][:, 2:3], dense[1][1])
    check(dense, LR.kl(xs[:, 2:3], xt[:, 2:3], T), f"channel slice T={T}")
    vessel = sliced(lambda a, b: losses.kl_loss_compute1(a[:, 2], b[:, 2], T))      # [N,D,H,W] maps of the same channel
    assert torch.equal(vessel[0], got[0]) and all(torch.equal(x, y) for x, y in zip(vessel[1], got[1]))


@pytest.mark.parametrize("student_ndhwc", [False, True])
def test_kl_mixed_layouts(student_ndhwc):
    ys, yt = _kl_pair(torch.Generator().manual_seed(67), 2, 8, SMALL)
    a, b = (ndhwc(ys), yt) if student_ndhwc else (ys, ndhwc(yt))
    assert a.stride() != b.stride()
    check(dev_loss(lambda s, t: losses.l2_loss(s, t, True, 4), [a, b]), LR.kl(ys, yt, 4, "l2"),
          f"mixed layouts, student NDHWC={student_ndhwc}")


@pytest.mark.parametrize("layout", ["planar", "ndhwc"])      # k_kl and k_kl_rows
@pytest.mark.parametrize("need", [(True, False), (False, True)])
def test_kl_one_sided_gradients(need, layout):
    ys, yt = _kl_pair(torch.Generator().manual_seed(71), 2, 8, SMALL)
    a, b = (ndhwc(ys), ndhwc(yt)) if layout == "ndhwc" else (ys, yt)
    got = dev_loss(lambda s, t: losses.distill_kl(s, t, 4), [a, b], need=need)
    assert [x is not None for x in got[1]] == list(need)
    check(got, LR.kl(ys, yt, 4, need=need), f"one-sided gradient {need} {layout}")


@pytest.mark.parametrize("layout", ["planar", "ndhwc"])
def test_kl_confident_teacher(layout):
    ys, yt = _kl_pair(torch.Generator().manual_seed(73), 2, 8, SMALL)
    yt = yt * 30.0
    assert bool((torch.softmax(yt, 1) == 0).any())      # some teacher probabilities underflow in fp32
    a, b = (ndhwc(ys), ndhwc(yt)) if layout == "ndhwc" else (ys, yt)
    check(dev_loss(lambda s, t: losses.distill_kl(s, t, 1), [a, b]), LR.kl(ys, yt, 1), f"confident teacher {layout}")


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("C", [4, 8, 16, 32])
def test_kl_row_kernel(C, T):
    """fp32 NDHWC rows: 1, 2, 4, 8 lanes per voxel; 630 rows are no multiple of the 256, 128, 64, 32 rows of a block"""
    ys, yt = _kl_pair(torch.Generator().manual_seed(80 + C), 2, C, SMALL)
    got = dev_loss(lambda a, b: losses.l2_loss(a, b, True, T), [ndhwc(ys), ndhwc(yt)])
    assert all(x.is_contiguous(memory_format=CL3D) for x in got[1])
    check(got, LR.kl(ys, yt, T, "l2"), f"k_kl_rows C={C} T={T}")


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("C", [4, 8, 16, 32])
def test_kl_row_kernel_grid_stride_loop(C, T):
    # mvd_kl_fwd: at most 2048 blocks of 256 / (C/4) rows; mvd_kl_bwd (k_kl_rows): grid_for(rows * C/4, 8192), i.e. at
    # most 8192 blocks of 256 lanes = 2 097 152 lanes; N * C = 128 gives 128 * 68 921 / 4 = 2 205 472 lanes for every C
    N = 128 // C
    ys, yt = _kl_pair(torch.Generator().manual_seed(90 + C), N, C, BIG)
    check(dev_loss(lambda a, b: losses.l2_loss(a, b, True, T), [ndhwc(ys), ndhwc(yt)]), LR.kl(ys, yt, T, "l2"),
          f"k_kl_rows [{N},{C},41^3] T={T}")


@pytest.mark.parametrize("C", [4, 32])
def test_kl_misaligned_rows_take_the_generic_kernel(C):
    """dense NDHWC rows that start one float into a buffer: k_kl_rows' 16-byte loads do not apply, mvd_kl_fwd / _bwd fall
    back to k_kl (another summation tree: no bit-equality with the aligned run, the same bars against fp64)"""
    ys, yt = _kl_pair(torch.Generator().manual_seed(97 + C), 2, C, SMALL)

    def run():
        a, b = misaligned(ndhwc(ys)).requires_grad_(True), misaligned(ndhwc(yt)).requires_grad_(True)
        l = losses.l2_loss(a, b, True, 4)
        l.backward()
        torch.cuda.synchronize()
        return l.detach().cpu(), [a.grad.cpu(), b.grad.cpu()]
    check(twice(run), LR.kl(ys, yt, 4, "l2"), f"misaligned NDHWC rows C={C}")


# ================================================================================================ 5. MSE
def test_mse_grid_stride_loops_and_tail():
    # mvd_mse_fwd: at most 4096 blocks of 256 float4 = 4 194 304 elements per trip, mvd_mse_bwd: 2048 blocks of 256
    # elements; n = 5 * 13 * 41^3 = 4 479 865 is odd: both loops take a second trip and one element is left for the tail
    g = torch.Generator().manual_seed(101)
    a, b = torch.randn((5, 13, *BIG), generator=g), torch.randn((5, 13, *BIG), generator=g) * 0.5 + 0.1
    assert a.numel() == 4479865 and a.numel() > 4 * 256 * 4096
    check(dev_loss(lambda x, y: ops.MseFn.apply(x, y), [a, b]), LR.mse(a, b), "mse n=4479865")


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_mse_tiny(n):
    g = torch.Generator().manual_seed(103 + n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    check(dev_loss(lambda x, y: ops.MseFn.apply(x, y), [a, b]), LR.mse(a, b), f"mse n={n}")


@pytest.mark.parametrize("need", [(True, False), (False, True)])
def test_mse_one_sided_gradients(need):
    g = torch.Generator().manual_seed(107)
    a, b = torch.randn((2, 3, *SMALL), generator=g), torch.randn((2, 3, *SMALL), generator=g)
    got = dev_loss(lambda x, y: ops.MseFn.apply(x, y), [a, b], need=need)
    assert [x is not None for x in got[1]] == list(need)
    check(got, LR.mse(a, b, need=need), f"mse one-sided {need}")


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_mse_misaligned_operand(which):
    """k_mse_fwd keeps its 16-byte loads; MseFn moves a dense operand that is not 16-byte aligned to an aligned buffer"""
    g = torch.Generator().manual_seed(109)
    a, b = torch.randn((2, 8, *SMALL), generator=g), torch.randn((2, 8, *SMALL), generator=g)
    a, b = ndhwc(a), ndhwc(b)

    def run():
        x = (misaligned(a) if which in ("a", "both") else a.to(DEV)).requires_grad_(True)
        y = (misaligned(b) if which in ("b", "both") else b.to(DEV)).requires_grad_(True)
        l = ops.MseFn.apply(x, y)
        l.backward()
        torch.cuda.synchronize()
        return l.detach().cpu(), [x.grad.cpu(), y.grad.cpu()]
    got = twice(run)
    check(got, LR.mse(a, b), f"mse misaligned {which}")
    aligned = dev_loss(lambda x, y: ops.MseFn.apply(x, y), [a, b])      # the same kernel on the same values
    assert torch.equal(got[0], aligned[0]) and all(torch.equal(x, y) for x, y in zip(got[1], aligned[1]))


# ================================================================================================ 6. clDice tail
@pytest.mark.parametrize("smooth", [1.0, 1e-3])
@pytest.mark.parametrize("shape", [(1, 1, *SMALL), (1, 1, 63, 65, 65)])      # mvd_dot_sum (topo.hip): at most 1024 blocks of
def test_cldice_tail(shape, smooth):                                          # 256 = 262 144; 63 * 65 * 65 = 266 175, odd
    g = torch.Generator().manual_seed(113)
    sp, st, pr = (torch.rand(shape, generator=g) for _ in range(3))
    tg = (torch.rand(shape, generator=g) > 0.6).float()
    got = dev_loss(lambda a, b: ops.ClDiceFn.apply(a, tg.to(DEV), st.to(DEV), b, smooth), [sp, pr])
    check(got, LR.cldice_tail(sp, tg, st, pr, smooth), f"clDice tail n={sp.numel()} smooth={smooth}")


def test_cldice_tail_empty_skeleton():
    g = torch.Generator().manual_seed(127)
    shape = (1, 1, *SMALL)
    st, pr = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    sp, tg = torch.zeros(shape), (torch.rand(shape, generator=g) > 0.6).float()
    got = dev_loss(lambda a, b: ops.ClDiceFn.apply(a, tg.to(DEV), st.to(DEV), b, 1.0), [sp, pr])
    check(got, LR.cldice_tail(sp, tg, st, pr, 1.0), "clDice tail, empty predicted skeleton")
