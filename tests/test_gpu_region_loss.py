"""GPU tests of the region / ignore-label losses (csrc/loss_region.hip, losses.DC_and_BCE_loss, DC_and_CE_loss(ignore_label=);
DESIGN 17) against the fp64 restatement tests/region_loss_ref.py.  Bars are the project's: loss 1e-5 relative,
gradients 1e-5 * max|g|; bit-exactness where the design promises it."""
import ctypes

import numpy as np
import pytest
import torch

import region_loss_ref as RR
from multimodal_mvd_seg_amd import losses, ops
from multimodal_mvd_seg_amd._lib import call, query

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
LOSS_TOL, GRAD_TOL = 1e-5, 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def regions_for(R):
    """R nested regions over the labels 1..R (region r = labels r+1..R), R = 1: one region of two labels"""
    if R == 1:
        return [(1, 2)], 3
    return [tuple(range(r + 1, R + 1)) if r + 1 < R else R for r in range(R)], R + 1


def make(seed, N, R, shape, nlab, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((N, R, *shape), generator=g) * scale
    seg = torch.randint(0, nlab, (N, 1, *shape), generator=g).float()
    return z, seg


def run_dev(loss, z, target):
    zd = [t.to(DEV).requires_grad_(True) for t in z] if isinstance(z, list) else z.to(DEV).requires_grad_(True)
    td = [t.to(DEV) for t in target] if isinstance(target, list) else target.to(DEV)
    l = loss(zd, td)
    l.backward()
    torch.cuda.synchronize()
    gr = [t.grad.cpu() for t in zd] if isinstance(z, list) else zd.grad.cpu()
    return l.detach().cpu(), gr


def run_ref(fn, z):
    zz = [t.double().requires_grad_(True) for t in z] if isinstance(z, list) else z.double().requires_grad_(True)
    l = fn(zz)
    l.backward()
    return l.detach(), ([t.grad for t in zz] if isinstance(z, list) else zz.grad)


def check(got, want, what):
    (l, g), (lr, gr) = got, want
    lerr = abs(float(l) - float(lr)) / max(abs(float(lr)), 1e-300)
    gs = g if isinstance(g, list) else [g]
    grs = gr if isinstance(gr, list) else [gr]
    gmax = max(float(x.abs().max()) for x in grs)
    gerr = max(float((a.double() - b).abs().max()) for a, b in zip(gs, grs))
    print(f"{what}: loss {float(l):.8f} ref {float(lr):.8f} rel {lerr:.2e}; grad err {gerr:.2e} of max|g| {gmax:.2e}")
    assert np.isfinite(float(l))
    assert lerr <= LOSS_TOL, lerr
    assert gerr <= GRAD_TOL * gmax, (gerr, gmax)


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_region_loss_matches_the_restatement(R, batch_dice, ignore):
    regions, ign = regions_for(R)
    ign = ign if ignore else None
    z, seg = make(10 + R, 2, R, (5, 7, 9), (ign + 1) if ignore else regions_for(R)[1])   # V = 315: no multiple of 4 or 256
    kw = {'batch_dice': batch_dice, 'do_bg': True, 'smooth': 1e-5, 'ddp': False}
    loss = losses.DC_and_BCE_loss({}, kw, use_ignore_label=ignore, regions=regions, ignore_label=ign)
    want = run_ref(lambda zz: RR.dc_and_bce_labelmap(zz, seg, regions, ign, batch_dice=batch_dice), z)
    check(run_dev(loss, z, seg), want, f"R={R} batch_dice={batch_dice} ignore={ignore}")


@pytest.mark.parametrize("ignore", [False, True])
def test_region_loss_full_resolution_level(ignore):
    regions, ign = [(1, 2, 3), (2, 3), 3], (4 if ignore else None)
    z, seg = make(3, 2, 3, (128, 128, 128), 5 if ignore else 4)
    loss = losses.DC_and_BCE_loss({}, {'batch_dice': True, 'do_bg': True, 'smooth': 1e-5, 'ddp': False},
                                  use_ignore_label=ignore, regions=regions, ignore_label=ign)
    want = run_ref(lambda zz: RR.dc_and_bce_labelmap(zz, seg, regions, ign, batch_dice=True), z)
    check(run_dev(loss, z, seg), want, f"[2,3,128^3] ignore={ignore}")


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("batch_dice", [False, True])
def test_label_map_form_equals_plane_form_bit_for_bit(batch_dice, ignore):
    regions, ign = [(1, 2, 3), (2, 3), 3], (4 if ignore else None)
    z, seg = make(4, 2, 3, (9, 11, 13), 5 if ignore else 4)
    kw = {'batch_dice': batch_dice, 'do_bg': True, 'smooth': 1e-5, 'ddp': False}
    la, ga = run_dev(losses.DC_and_BCE_loss({}, kw, use_ignore_label=ignore, regions=regions, ignore_label=ign), z, seg)
    planes_dev = ops.convert_seg_to_regions(seg.to(DEV), regions, ign).cpu()
    planes = torch.from_numpy(RR.seg_to_regions(seg.numpy(), regions, ign))
    assert torch.equal(planes_dev, planes)    # the device transform is the reference's transform
    lb, gb = run_dev(losses.DC_and_BCE_loss({}, kw, use_ignore_label=ignore), z, planes)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    check((lb, gb), run_ref(lambda zz: RR.dc_and_bce(zz, planes, ignore, batch_dice=batch_dice), z), "planes")


def test_sample_with_every_voxel_ignored():
    regions, ign = [(1, 2, 3), (2, 3), 3], 4
    z, seg = make(5, 2, 3, (6, 7, 8), 4)
    seg[0] = ign
    kw = {'batch_dice': False, 'do_bg': True, 'smooth': 1e-5, 'ddp': False}
    loss = losses.DC_and_BCE_loss({}, kw, use_ignore_label=True, regions=regions, ignore_label=ign)
    l, g = run_dev(loss, z, seg)
    assert np.isfinite(float(l)) and bool((g[0] == 0).all()) and bool((g[1] != 0).any())
    check((l, g), run_ref(lambda zz: RR.dc_and_bce_labelmap(zz, seg, regions, ign), z), "one sample ignored")
    seg[:] = ign   # the whole batch: BCE term 0 (not NaN), gradient exactly zero
    l, g = run_dev(losses.DC_and_BCE_loss({}, kw, weight_dice=0, use_ignore_label=True, regions=regions, ignore_label=ign), z, seg)
    assert float(l) == 0.0 and bool((g == 0).all())
    l, g = run_dev(loss, z, seg)
    assert np.isfinite(float(l)) and bool((g == 0).all())
    # softmax heads: CE term 0 when no voxel is valid
    z4, seg4 = make(6, 2, 4, (6, 7, 8), 4)
    seg4[:] = 4
    ce = losses.DC_and_CE_loss({'batch_dice': False, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}, weight_dice=0,
                               ignore_label=4)
    l, g = run_dev(ce, z4, seg4)
    assert float(l) == 0.0 and bool((g == 0).all())
    both = losses.DC_and_CE_loss({'batch_dice': False, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}, ignore_label=4)
    l, g = run_dev(both, z4, seg4)
    assert np.isfinite(float(l)) and bool((g == 0).all())


@pytest.mark.parametrize("batch_dice", [False, True])
def test_empty_region(batch_dice):
    regions = [(1, 2), 2, 3]      # label 3 never occurs: G = 0 for the last head
    z, seg = make(7, 2, 3, (6, 7, 8), 3)
    kw = {'batch_dice': batch_dice, 'do_bg': True, 'smooth': 1e-5, 'ddp': False}
    want = run_ref(lambda zz: RR.dc_and_bce_labelmap(zz, seg, regions, None, batch_dice=batch_dice), z)
    check(run_dev(losses.DC_and_BCE_loss({}, kw, regions=regions), z, seg), want, "empty region")


@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("K", [2, 5])
def test_masked_dc_and_ce(K, batch_dice):
    z, seg = make(20 + K, 2, K, (5, 7, 9), K + 1)     # label K is the ignore label
    kw = {'batch_dice': batch_dice, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}
    want = run_ref(lambda zz: RR.dc_and_ce_masked(zz, seg, K, batch_dice=batch_dice), z)
    check(run_dev(losses.DC_and_CE_loss(kw, {}, ignore_label=K), z, seg), want, f"masked CE K={K}")
    # no voxel ignored: the value of the plain loss to the same bars
    seg2 = seg.clamp(max=K - 1)
    want = run_ref(lambda zz: RR.dc_and_ce_masked(zz, seg2, None, batch_dice=batch_dice), z)
    check(run_dev(losses.DC_and_CE_loss(kw, {}, ignore_label=K), z, seg2), want, f"masked CE K={K}, nothing ignored")


@pytest.mark.parametrize("mode", ["regions", "regions+ignore", "ignore"])
def test_deep_supervision_wrapper(mode):
    shapes = [(16, 16, 16), (8, 8, 8), (4, 4, 4)]
    w = losses.ds_weights(3)
    assert w[-1] == 0
    regions = [(1, 2, 3), (2, 3), 3]
    ign = None if mode == "regions" else 4
    C = 4 if mode == "ignore" else 3
    zs, ts = [], []
    for i, s in enumerate(shapes):
        z, seg = make(30 + i, 2, C, s, 4 if ign is None else 5)
        zs.append(z)
        ts.append(seg)
    if mode == "ignore":
        base = losses.DC_and_CE_loss({'batch_dice': True, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}, ignore_label=ign)
        fn = lambda o, t: RR.dc_and_ce_masked(o, t, ign, batch_dice=True)
    else:
        base = losses.DC_and_BCE_loss({}, {'batch_dice': True, 'do_bg': True, 'smooth': 1e-5, 'ddp': False},
                                      use_ignore_label=ign is not None, regions=regions, ignore_label=ign)
        fn = lambda o, t: RR.dc_and_bce_labelmap(o, t, regions, ign, batch_dice=True)
    l, g = run_dev(losses.DeepSupervisionWrapper(base, w), zs, ts)
    assert bool((g[-1] == 0).all())     # the zero-weight level: an exact-zero gradient, not None
    want = run_ref(lambda zz: RR.deep_supervised(fn, zz, ts, [float(x) for x in w]), zs)
    check((l, g[:-1]), (want[0], want[1][:-1]), f"deep supervision {mode}")


def test_twelve_repetitions_are_bit_identical():
    regions, ign = [(1, 2, 3), (2, 3), 3], 4
    z, seg = make(8, 2, 3, (40, 41, 43), 5)
    bce = losses.DC_and_BCE_loss({}, {'batch_dice': True, 'do_bg': True, 'smooth': 1e-5, 'ddp': False},
                                 use_ignore_label=True, regions=regions, ignore_label=ign)
    z4, seg4 = make(9, 2, 4, (40, 41, 43), 5)
    ce = losses.DC_and_CE_loss({'batch_dice': False, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}, ignore_label=4)
    for loss, zz, tt in ((bce, z, seg), (ce, z4, seg4)):
        first = run_dev(loss, zz, tt)
        for _ in range(11):
            again = run_dev(loss, zz, tt)
            assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_plain_path_is_the_direct_dcce_call_sequence():
    """The unmasked DC_and_CE_loss still issues mvd_dcce_fwd / finalize / bwd and nothing else: bit-identical."""
    z, seg = make(11, 2, 4, (17, 19, 23), 4)
    for bd in (False, True):
        l, g = run_dev(losses.DC_and_CE_loss({'batch_dice': bd, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}), z, seg)
        x, t = z.to(DEV).contiguous(), seg.to(DEV).reshape(2, -1).contiguous()
        N, K, V = 2, 4, t.shape[1]
        p = lambda a: ctypes.c_void_p(a.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        stats = torch.empty((N, 3 * K + 1), device=DEV)
        ws = torch.empty(query("mvd_dcce_workspace_bytes", N, V, K), dtype=torch.uint8, device=DEV)
        call("mvd_dcce_fwd", p(x), p(t), p(stats), N, V, K, p(ws), ws.numel(), st)
        loss, coef = torch.empty(3, device=DEV), torch.empty((N, K, 2), device=DEV)
        call("mvd_dcce_finalize", p(stats), N, p(stats), N, p(loss), p(coef), V, K, int(bd), 0, 1e-5, 1.0, 1.0, st)
        dl, one = torch.empty_like(x), torch.ones(1, device=DEV)
        call("mvd_dcce_bwd", p(x), p(t), p(coef), p(one), 1.0, p(dl), N, V, K, 1.0, st)
        torch.cuda.synchronize()
        assert torch.equal(l, loss[0].cpu()) and torch.equal(g, dl.cpu())


def test_more_heads_than_the_kernels_hold_is_refused():
    z = torch.zeros((1, 9, 4, 4, 4), device=DEV)
    with pytest.raises(NotImplementedError, match="at most 8"):
        losses.DC_and_BCE_loss({}, {})(z, torch.zeros((1, 9, 4, 4, 4), device=DEV))
