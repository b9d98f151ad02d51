"""GPU tests of the top-k cross entropy (csrc/loss_topk.hip, ops.DeepSupervisedTopKFn, losses.TopKLoss / DC_and_topk_loss)
against tests/topk_ref.py in fp64.

Bars: loss 1e-5 relative, gradients 1e-5 of the reference's largest magnitude per tensor; the integers of
the selection (t_bits, cnt_gt, cnt_eq against a host sort of the device's own ce buffer) bit-exact; every device
evaluation runs twice and repeats bit for bit.

Boundary band: a voxel whose fp64 CE lies within 1e-5 * t of the threshold t may be selected differently by fp32
arithmetic, and its gradient row then differs by the whole CE row.  For such voxels either valid row is accepted (the
voxel selected, or not selected: an exact zero for the plain top-k), every other voxel is held to the bar, and on tie-free
inputs exactly k rows must be non-zero.  The band is capped at 2 voxels on the small shapes and 32 on the large one (it
holds the k-th element itself: at least 1).  Shapes and the launch caps they cross: DESIGN 29."""
import numpy as np
import pytest
import torch

import topk_ref as TR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMALL = (5, 7, 9)        # V = 315: no multiple of 4 or 256; n = 315 / 945 -> k = 31 / 94
BIG = (41, 41, 41)       # V = 68 921 (odd), N = 16: every new wrapper's block cap is crossed
LOSS_BAR, GRAD_BAR, BAND = 1e-5, 1e-5, 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def inputs(seed, N, K, shape, scale=2.0):
    torch.manual_seed(seed)
    z = torch.randn(N, K, *shape) * scale
    t = torch.randint(0, K, (N, 1, *shape)).float()
    return z, t


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two evaluations of the same device call differ"
    return a


def dev_eval(fn, zs, scale=None):
    """-> loss, grad per logits tensor (CPU), evaluated twice"""
    def run():
        xs = [z.to(DEV).requires_grad_(True) for z in zs]
        l = fn(*xs)
        (l if scale is None else l * scale).backward()
        torch.cuda.synchronize()
        return [l.detach().cpu()] + [x.grad.cpu() for x in xs]
    out = twice(run)
    return out[0], out[1:]


def reference(z, t, ign=-100, eps=0.0, k_percent=10, dice=None, scale=1.0, dice_extra=None, mult=1.0):
    """fp64: loss, gradient, and what the band check needs.  dice = dict(batch_dice, do_bg, smooth, w_ce, w_dice,
    ignore_label); dice_extra = (z_other, t_other) put in front of the local batch for the Dice half, whose gradient is
    multiplied by `mult` (the stub gather)."""
    zz = z.double().requires_grad_(True)
    ltk, ce, thr, cnt_gt, cnt_eq, w = TR.topk_loss(zz, t, k_percent, ign, eps, parts=True)
    k = TR.topk_count(ce.numel(), k_percent)
    w_ce = 1.0
    g = torch.zeros_like(zz)
    total = ltk
    if dice is not None:
        w_ce = dice["w_ce"]
        zd, td = zz, t
        if dice_extra is not None:
            zd, td = torch.cat([dice_extra[0].double(), zz]), torch.cat([dice_extra[1], t])
        dl = TR.dc_and_topk(zz, t, dice["ignore_label"], dice["batch_dice"], dice["do_bg"], dice["smooth"], 0.0, dice["w_dice"],
                            k_percent, eps, dice_z=zd, dice_target=td)
        g = g + mult * torch.autograd.grad(dl, zz, retain_graph=True)[0]
        total = w_ce * ltk + dl
    g = (g + w_ce * torch.autograd.grad(ltk, zz, retain_graph=True)[0]) * scale
    rows, = torch.autograd.grad(TR.ce_per_voxel(zz, t, ign, eps).sum(), zz)
    return dict(loss=float(total), g=g.detach(), rows=rows * (w_ce * scale / k), ce=ce, thr=float(thr), cnt_gt=cnt_gt,
                cnt_eq=cnt_eq, w=w, k=k, valid=(t[:, 0] != ign))


def check(got_loss, got_g, ref, what, band_cap=2, ties=False, count_rows=False):
    lerr = abs(float(got_loss) - ref["loss"]) / max(abs(ref["loss"]), 1e-30)
    bar = GRAD_BAR * float(ref["g"].abs().max())
    d = got_g.double()
    err = (d - ref["g"]).abs().amax(1)                         # [N, *spatial]
    near = ((ref["ce"] - ref["thr"]).abs() <= BAND * ref["thr"]) & ref["valid"]
    nband = int(near.sum())
    if ties:
        band = torch.zeros_like(near)                         # exact ties: the share is held to the bar like everything else
    else:
        band = near
        assert nband <= band_cap and (nband >= 1 or ref["thr"] == 0.0), f"{what}: band of {nband} voxels"
    sel = (d - (ref["g"] + ((1.0 - ref["w"] * ref["k"])[:, None]) * ref["rows"])).abs().amax(1)
    uns = (d - (ref["g"] + ((0.0 - ref["w"] * ref["k"])[:, None]) * ref["rows"])).abs().amax(1)
    err = torch.where(band, torch.minimum(sel, uns), err)
    gerr = float(err.max())
    print(f"{what}: loss {float(got_loss):.7f} ref {ref['loss']:.7f} rel {lerr:.2e}; grad err {gerr:.2e} bar {bar:.2e}; "
          f"k {ref['k']} cnt_gt {ref['cnt_gt']} cnt_eq {ref['cnt_eq']} band {nband}")
    assert lerr <= LOSS_BAR, (what, lerr)
    assert gerr <= bar, (what, gerr, bar)
    if count_rows:
        assert int((got_g != 0).any(1).sum()) == ref["k"], f"{what}: {int((got_g != 0).any(1).sum())} non-zero rows, k = {ref['k']}"


def check_state(z, t, ign, eps, k_percent=10):
    """t_bits, cnt_gt, cnt_eq of the device against a host sort of the device's own ce buffer: bit-exact"""
    from multimodal_mvd_seg_amd import ops
    ce = ops.topk_ce(z.to(DEV), t.to(DEV), ign, eps)
    k = ops.topk_count(ce.numel(), k_percent)
    a, b = ops.topk_select(ce, k).cpu().numpy(), ops.topk_select(ce, k).cpu().numpy()
    assert np.array_equal(a, b)
    _check_select(ce.cpu().numpy().reshape(-1), k, a)
    c = ce.cpu().numpy()
    assert not np.signbit(c).any() and np.all(c[(t[:, 0] == ign).reshape(c.shape).numpy()] == 0)
    return a


def _check_select(c, k, got):
    bits = c.view(np.uint32).astype(np.int64)
    tb = np.sort(bits)[::-1][k - 1]
    want = np.array([tb, (bits > tb).sum(), (bits == tb).sum()], dtype=np.int64)
    assert np.array_equal(got, want), (got, want)


# ------------------------------------------------------------------------------------------------ the loss, small shapes
@pytest.mark.parametrize("K", [2, 3, 5, 8])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("case", ["plain", "smooth", "ignore_few", "ignore_most", "ignore_smooth"])
def test_topk_small(case, N, K):
    from multimodal_mvd_seg_amd import losses
    z, t = inputs(K % 3, N, K, SMALL)
    eps = 0.1 if "smooth" in case else 0.0
    ign = K if "ignore" in case else -100
    if "ignore" in case:
        frac = {"ignore_few": 0.05, "ignore_most": 0.95, "ignore_smooth": 0.3}[case]
        t[torch.rand(t.shape, generator=torch.Generator().manual_seed(7)) < frac] = float(K)
    ref = reference(z, t, ign, eps)
    if case == "ignore_most":   # fewer valid voxels than k: the threshold is 0 and ties against the ignored zeros
        assert int(ref["valid"].sum()) < ref["k"] and ref["thr"] == 0.0 and ref["cnt_eq"] > 1
    loss_fn = losses.TopKLoss(ignore_index=ign, k=10, label_smoothing=eps)
    l, (g,) = dev_eval(lambda x: loss_fn(x, t.to(DEV)), [z])
    check(l, g, ref, f"{case} N={N} K={K}", count_rows=case != "ignore_most")
    st = check_state(z, t, ign, eps)
    if case == "ignore_most":
        assert st[0] == 0
    assert bool((g.movedim(1, -1)[~ref["valid"]] == 0).all())       # ignored voxels: exact zeros


def test_k_is_1_and_k_is_0():
    from multimodal_mvd_seg_amd import losses
    z, t = inputs(1, 1, 2, (2, 2, 3))          # n = 12 -> k = 1
    ref = reference(z, t)
    assert ref["k"] == 1 and ref["cnt_gt"] == 0 and ref["cnt_eq"] == 1
    l, (g,) = dev_eval(lambda x: losses.TopKLoss()(x, t.to(DEV)), [z])
    check(l, g, ref, "k == 1", count_rows=True)
    assert check_state(z, t, -100, 0.0)[1] == 0
    z0, t0 = inputs(1, 1, 2, (1, 3, 3))        # n = 9 -> k = 0
    with pytest.raises(ValueError, match=r"k = int\(9 voxels \* 10 / 100\) = 0"):
        losses.TopKLoss()(z0.to(DEV), t0.to(DEV))


def test_nine_classes_are_refused():
    from multimodal_mvd_seg_amd import losses
    z, t = inputs(0, 1, 9, (4, 4, 4))
    with pytest.raises(NotImplementedError, match="at most 8"):
        losses.TopKLoss()(z.to(DEV), t.to(DEV))
    with pytest.raises(NotImplementedError, match="at most 8"):
        losses.DC_and_topk_loss({}, {})(z.to(DEV), t.to(DEV))


@pytest.mark.parametrize("K", [2, 5, 8])
def test_all_logits_zero(K):
    """every CE equal: one histogram bin at every pass (the LDS-contention worst case), cnt_gt == 0, all voxels tied"""
    from multimodal_mvd_seg_amd import losses
    z, t = inputs(0, 3, K, SMALL)
    z.zero_()
    ref = reference(z, t)
    assert ref["cnt_gt"] == 0 and ref["cnt_eq"] == 945 and abs(ref["loss"] - np.log(K)) < 1e-14
    l, (g,) = dev_eval(lambda x: losses.TopKLoss()(x, t.to(DEV)), [z])
    check(l, g, ref, f"all-equal K={K}", ties=True)
    st = check_state(z, t, -100, 0.0)
    assert st[1] == 0 and st[2] == 945


def test_logits_times_40():
    """CE from exact 0 to about 300: the threshold lies far from the top bin, zeros at the bottom"""
    from multimodal_mvd_seg_amd import losses, ops
    z, t = inputs(2, 3, 5, SMALL, scale=80.0)
    ref = reference(z, t)
    l, (g,) = dev_eval(lambda x: losses.TopKLoss()(x, t.to(DEV)), [z])
    check(l, g, ref, "logits x 40", count_rows=True)
    check_state(z, t, -100, 0.0)
    ce = ops.topk_ce(z.to(DEV), t.to(DEV)).cpu()
    assert float(ce.min()) == 0.0 and float(ce.max()) > 100.0


def test_upstream_gradient_scale():
    from multimodal_mvd_seg_amd import losses
    z, t = inputs(1, 3, 5, SMALL)
    ref = reference(z, t, eps=0.1, scale=2.5)
    l, (g,) = dev_eval(lambda x: losses.TopKLoss(label_smoothing=0.1)(x, t.to(DEV)), [z], scale=2.5)
    check(l, g, ref, "upstream gradient 2.5", count_rows=True)


def _tie(z, t, ref, above, below):
    """copy the k-th voxel's logits and label over `above` voxels from above the threshold and `below` from below it"""
    N, K = z.shape[:2]
    zf, tf = z.reshape(N, K, -1).clone(), t.reshape(N, -1).clone()
    order = torch.argsort(ref["ce"].reshape(-1), descending=True)
    V = zf.shape[2]
    src = int(order[ref["k"] - 1])
    dst = [int(order[i]) for i in range(2, 2 + above)] + [int(order[ref["k"] + 5 + 3 * i]) for i in range(below)]
    for d in dst:
        zf[d // V, :, d % V] = zf[src // V, :, src % V]
        tf[d // V, d % V] = tf[src // V, src % V]
    return zf.reshape(z.shape), tf.reshape(t.shape), [src] + dst


@pytest.mark.parametrize("above,below", [(0, 1), (2, 4)])
def test_exact_ties_at_the_threshold_share_the_rest(above, below):
    from multimodal_mvd_seg_amd import losses
    z, t = inputs(0, 3, 5, SMALL)
    z, t, tied = _tie(z, t, reference(z, t), above, below)
    ref = reference(z, t)
    k = ref["k"]
    assert ref["cnt_eq"] == 1 + above + below and ref["cnt_gt"] == k - 1 - above
    # nothing but the tied voxels lies in the band, so every row is held to the bar
    assert int((((ref["ce"] - ref["thr"]).abs() <= BAND * ref["thr"])).sum()) == ref["cnt_eq"]
    l, (g,) = dev_eval(lambda x: losses.TopKLoss()(x, t.to(DEV)), [z])
    check(l, g, ref, f"ties {above}+{below}", ties=True)
    st = check_state(z, t, -100, 0.0)
    assert (st[1], st[2]) == (ref["cnt_gt"], ref["cnt_eq"])
    rows = g.reshape(3, 5, -1)
    V = rows.shape[2]
    first = rows[tied[0] // V, :, tied[0] % V]
    assert bool(first.abs().max() > 0)
    for d in tied[1:]:
        assert torch.equal(rows[d // V, :, d % V], first)        # the same share on every tied voxel, bit for bit
    share = (k - ref["cnt_gt"]) / ref["cnt_eq"]
    full = ref["rows"].reshape(3, 5, -1)[tied[0] // V, :, tied[0] % V]
    assert float((first.double() - share * full).abs().max()) <= GRAD_BAR * float(ref["g"].abs().max())


def test_three_levels_one_of_them_zero_weight():
    from multimodal_mvd_seg_amd import losses
    shapes = [(8, 10, 12), (4, 5, 6), (2, 3, 3)]
    zs, ts = zip(*[inputs(3 + i, 2, 4, s) for i, s in enumerate(shapes)])
    w = [0.5, 0.0, 0.5]
    wrapper = losses.DeepSupervisionWrapper(losses.TopKLoss(label_smoothing=0.1), w)
    l, gs = dev_eval(lambda *x: wrapper(list(x), [t.to(DEV) for t in ts]), list(zs), scale=2.5)
    refs = [reference(z, t, eps=0.1, scale=2.5 * wi) for z, t, wi in zip(zs, ts, w)]
    want = sum(wi * r["loss"] for wi, r in zip(w, refs))
    assert abs(float(l) - want) / abs(want) <= LOSS_BAR
    assert gs[1].shape == zs[1].shape and bool((gs[1] == 0).all())       # zero weight: exact zeros, not None
    for i in (0, 2):
        # (the total was checked above: check() looks at the gradient of level i)
        check(l, gs[i], dict(refs[i], loss=float(l)), f"level {i}", count_rows=True)


# ------------------------------------------------------------------------------------------------ DC_and_topk
def _dice_cfg(batch_dice, do_bg, w_ce, w_dice, ign):
    return dict(batch_dice=batch_dice, do_bg=do_bg, smooth=1e-5, w_ce=w_ce, w_dice=w_dice, ignore_label=ign)


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.3, 1.7)])
@pytest.mark.parametrize("do_bg", [False, True])
@pytest.mark.parametrize("batch_dice", [False, True])
def test_dc_and_topk(batch_dice, do_bg, weights, ignore):
    from multimodal_mvd_seg_amd import losses
    K = 5
    z, t = inputs(1, 3, K, SMALL)
    ign = K if ignore else None
    if ignore:
        t[torch.rand(t.shape, generator=torch.Generator().manual_seed(11)) < 0.2] = float(K)
    cfg = _dice_cfg(batch_dice, do_bg, *weights, ign)
    ref = reference(z, t, K if ignore else -100, 0.0, dice=cfg, scale=2.5)
    loss_fn = losses.DC_and_topk_loss({'batch_dice': batch_dice, 'do_bg': do_bg, 'smooth': 1e-5, 'ddp': False},
                                      {'k': 10, 'label_smoothing': 0.0}, weight_ce=weights[0], weight_dice=weights[1],
                                      ignore_label=ign)
    l, (g,) = dev_eval(lambda x: loss_fn(x, t.to(DEV)), [z], scale=2.5)
    check(l, g, ref, f"DC_and_topk batch_dice={batch_dice} do_bg={do_bg} w={weights} ignore={ignore}")
    assert bool((g.movedim(1, -1)[~ref["valid"]] == 0).all())


@pytest.mark.parametrize("ignore", [False, True])
def test_dc_and_topk_stub_gather(ignore):
    """the Dice statistics of a second batch in front of the local ones (Nd = 5 != N = 2, off = 3), gradient multiplier 2;
    the top-k stays local"""
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd.ops import _Workspace, _p, _stream, call, query
    K = 5
    z, t = inputs(2, 2, K, SMALL)
    zo, to = inputs(5, 3, K, SMALL)
    ign = K if ignore else None
    if ignore:
        t[torch.rand(t.shape, generator=torch.Generator().manual_seed(12)) < 0.2] = float(K)
        to[torch.rand(to.shape, generator=torch.Generator().manual_seed(13)) < 0.2] = float(K)
    xo, tt = zo.to(DEV).contiguous(), to.to(DEV).reshape(3, -1).contiguous()
    V = tt.shape[1]
    stats_other = torch.empty((3, 3 * K + (2 if ignore else 1)), device=DEV)
    if ignore:
        ws = _Workspace.get(query("mvd_dcce_masked_workspace_bytes", 3, V, K), DEV)
        call("mvd_dcce_masked_fwd", _p(xo), _p(tt), _p(stats_other), 3, V, K, K, _p(ws), ws.numel(), _stream())
    else:
        ws = _Workspace.get(query("mvd_dcce_workspace_bytes", 3, V, K), DEV)
        call("mvd_dcce_fwd", _p(xo), _p(tt), _p(stats_other), 3, V, K, _p(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    seen = []

    def gather(stats):
        seen.append(tuple(stats.shape))
        return torch.cat([stats_other, stats]), 3, 2.0
    cfg = _dice_cfg(True, False, 0.3, 1.7, ign)
    dev_cfg = (10, 0.0, K if ignore else -100, (True, False, 1e-5, 0.3, 1.7, ign))
    l, (g,) = dev_eval(lambda x: ops.DeepSupervisedTopKFn.apply([1.0], dev_cfg, gather, [t.to(DEV)], x), [z])
    assert seen == [(2, stats_other.shape[1])] * 2
    ref = reference(z, t, K if ignore else -100, 0.0, dice=cfg, dice_extra=(zo, to), mult=2.0)
    check(l, g, ref, f"stub gather ignore={ignore}")


# ------------------------------------------------------------------------------------------------ the selection alone
def _select_case(name, n):
    g = np.random.default_rng(len(name) + n)
    if name == "one_first_pass_bin":       # [1, 1.25): threshold in the highest AND the lowest occupied bin of pass 0
        return (1.0 + 0.25 * g.random(n)).astype(np.float32)
    if name == "wide":                     # zeros, denormals, and everything up to 3e38
        c = np.exp(g.uniform(-100, 88, n)).astype(np.float32)
        c[::7] = 0.0
        c[1::11] = 1e-42
        c[2::13] = 3e38
        return c
    if name == "few_distinct":             # heavy ties at every pass
        return g.choice(np.array([0.0, 0.5, 0.5000001, 2.0, 2.0000002, 7.0], dtype=np.float32), n)
    raise KeyError(name)


@pytest.mark.parametrize("n", [12, 315, 70001])
@pytest.mark.parametrize("name", ["one_first_pass_bin", "wide", "few_distinct"])
def test_select_equals_a_host_sort(name, n):
    """k from 1 (threshold in the highest occupied bin) to n (in the lowest); 70001 values: several workgroups"""
    from multimodal_mvd_seg_amd import ops
    c = _select_case(name, n)
    dev = torch.from_numpy(c).to(DEV)
    for k in sorted({1, 2, n // 10, n // 2, n - 1, n}):
        if k >= 1:
            _check_select(c, k, ops.topk_select(dev, k).cpu().numpy())
    with pytest.raises(RuntimeError, match="k == 0"):
        ops.topk_select(dev, 0)


# ------------------------------------------------------------------------------------------------ the launch caps
def test_topk_grid_stride_loops():
    """[16, 8, 41^3]: 270 blocks of voxels per sample against caps of 128 (ce_fwd) and 256 (bwd) per sample, n = 1 102 736
    values = 4308 blocks against 2048 (histograms) and 1024 (sum): every grid-stride loop runs more than once, and the
    last voxel of every sample sits in a partial block"""
    from multimodal_mvd_seg_amd import losses
    N, K = 16, 8
    z, t = inputs(0, N, K, BIG)
    t[torch.rand(t.shape, generator=torch.Generator().manual_seed(17)) < 0.05] = float(K)
    ref = reference(z, t, K, 0.1)
    l, (g,) = dev_eval(lambda x: losses.TopKLoss(ignore_index=K, label_smoothing=0.1)(x, t.to(DEV)), [z])
    check(l, g, ref, "grid-stride", band_cap=32, count_rows=True)
    check_state(z, t, K, 0.1)
