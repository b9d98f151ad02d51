"""k_fwd_wino3's output side: the exchange through LDS, the store addressing and the statistics epilogue, at the smallest
shapes where a misplaced element cannot hide.  (5, 9, 11) leaves the last 2x2x2 octet half outside along every axis, so
all eight output parities meet a boundary; small-integer data makes every comparison exact.  The 3-D engine is forced
with mvd_set_wino3_min_items(1) and restored in `finally`."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _skip_if_off():
    from multimodal_mvd_seg_amd._lib import call, i3, query
    if query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0: the Winograd engines are switched off for this run")
    try:
        call("mvd_set_wino_min_items", 1)
        call("mvd_set_wino3_min_items", 1)
        if not query("mvd_conv_wino3_applicable", 1, 8, 8, 8, 32, 0, 32, i3((3, 3, 3)), i3((1, 1, 1))):
            pytest.skip("MVD_WINO3=0: the 3-D engine is switched off for this run")
    finally:
        call("mvd_set_wino_min_items", -1)
        call("mvd_set_wino3_min_items", -1)


def _run(x1, x2, w, b, gy):
    """forward + input gradient through ops.Conv3dFn with the 3-D engine forced: y, dx1, dx2, (stats, ntiles)"""
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, i3, query
    try:
        call("mvd_set_wino_min_items", 1)
        call("mvd_set_wino3_min_items", 1)
        N, C1 = x1.shape[:2]
        C2 = x2.shape[1] if x2 is not None else 0
        bits3 = query("mvd_conv_wino3_applicable", N, *x1.shape[2:], C1, C2, w.shape[0], i3((3, 3, 3)), i3((1, 1, 1)))
        assert bits3 == 3, bits3
        g1 = x1.to(DEV).requires_grad_()
        g2 = x2.to(DEV).requires_grad_() if x2 is not None else None
        y = ops.Conv3dFn.apply(g1, g2, w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_(), (1, 1, 1))
        stats = getattr(y, "_mvd_tile_stats", None)
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
        return y.detach().cpu(), g1.grad.cpu(), (g2.grad.cpu() if x2 is not None else None), stats
    finally:
        call("mvd_set_wino_min_items", -1)
        call("mvd_set_wino3_min_items", -1)


def _integer_case(C1, C2, K, sp, N, seed):
    """|x| <= 2, |w| <= 1 (test_wino3_exact_integer_data): every partial sum of the kernel is an exact multiple of 1/8"""
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randint(-2, 3, (N, C1, *sp), generator=g).float()
    x2 = torch.randint(-2, 3, (N, C2, *sp), generator=g).float() if C2 else None
    w = torch.randint(-1, 2, (K, C1 + C2, 3, 3, 3), generator=g).float()
    b = torch.randint(-4, 5, (K,), generator=g).float()
    x = torch.cat([x1, x2], 1) if C2 else x1
    ref = F.conv3d(x.double(), w.double(), b.double(), 1, 1)
    gy = torch.randint(-2, 3, ref.shape, generator=g).float()
    refx = torch.nn.grad.conv3d_input(x.shape, w.double(), gy.double(), 1, 1)
    return x1, x2, w, b, gy, ref, refx


@pytest.mark.parametrize("C,K", [(32, 32), (64, 96)])
def test_wino3_epilogue_exact_one_pointer(C, K):
    """N = 2 at (5, 9, 11): the last octet is half outside along D, H and W.  (64, 96) has three k-blocks in the forward
    pass and two in the input gradient."""
    _skip_if_off()
    x, _, w, b, gy, ref, refx = _integer_case(C, 0, K, (5, 9, 11), 2, C + K)
    y, dx, _, _ = _run(x, None, w, b, gy)
    assert torch.equal(y.double(), ref), float((y.double() - ref).abs().max())
    assert torch.equal(dx.double(), refx), float((dx.double() - refx).abs().max())


def test_wino3_epilogue_exact_two_pointers():
    """32 + 32 -> 32 at (6, 10, 7), N = 2: two input tensors forward, and the input gradient writes two tensors."""
    _skip_if_off()
    x1, x2, w, b, gy, ref, refx = _integer_case(32, 32, 32, (6, 10, 7), 2, 11)
    y, d1, d2, _ = _run(x1, x2, w, b, gy)
    assert torch.equal(y.double(), ref), float((y.double() - ref).abs().max())
    assert torch.equal(d1.double(), refx[:, :32]), float((d1.double() - refx[:, :32]).abs().max())
    assert torch.equal(d2.double(), refx[:, 32:]), float((d2.double() - refx[:, 32:]).abs().max())


def _float_case():
    g = torch.Generator().manual_seed(15)
    N, C, K, sp = 2, 32, 64, (5, 9, 11)
    x = torch.randn(N, C, *sp, generator=g)
    w = torch.randn(K, C, 3, 3, 3, generator=g) / np.sqrt(27 * C)
    b = torch.randn(K, generator=g) * 0.1
    gy = torch.randn(N, K, *sp, generator=g)
    return x, w, b, gy, sp


def _plain_forward(x, w, b):
    """mvd_conv3d_fwd_routed with the 3-D table and without the statistics epilogue, on the tables ops.py would pack"""
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import CONV_WINO3, call, i3, query
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, C, D, H, W = x.shape
    K = w.shape[0]
    try:
        call("mvd_set_wino_min_items", 1)
        call("mvd_set_wino3_min_items", 1)
        assert query("mvd_conv_wino3_applicable", N, D, H, W, C, 0, K, i3((3, 3, 3)), i3((1, 1, 1))) == 3
        xd = ops.to_ndhwc(x.to(DEV))
        wd, bd = w.to(DEV), b.to(DEV)
        wf, _ = ops.pack_weight(wd, False)
        vf = torch.empty(query("mvd_wino3_weight_elems", C, K), device=DEV)
        vb = torch.empty(query("mvd_wino3_weight_elems", C, K), device=DEV)
        call("mvd_pack_weight_wino3", P(wd), P(vf), P(vb), K, C, s)
        y = ops.empty_cl3d((N, K, D, H, W), DEV)
        ws = torch.empty(max(query("mvd_conv_fwd_workspace_bytes", N, D * H * W, K), 1024), dtype=torch.uint8, device=DEV)
        call("mvd_conv3d_fwd_routed", P(xd), C, None, 0, P(wf), P(vf), CONV_WINO3, P(bd), P(y), None, 0, None, N, D, H, W, K,
             i3((3, 3, 3)), i3((1, 1, 1)), P(ws), ws.numel(), s)
        torch.cuda.synchronize()
        return y.cpu()
    finally:
        call("mvd_set_wino_min_items", -1)
        call("mvd_set_wino3_min_items", -1)


def test_wino3_epilogue_statistics_ragged_everywhere():
    """Per-tile (sum, sum of squares) against sums taken from the output itself at (5, 9, 11), N = 2, K = 64: D, H and W
    are all ragged, and H leaves the second 4-row half of the last 8-row tile with one row.  Bars of
    test_wino3_statistics_epilogue.  The statistics entry point's output equals the plain entry point's bit for bit."""
    _skip_if_off()
    from multimodal_mvd_seg_amd._lib import query
    x, w, b, gy, sp = _float_case()
    y, _, _, stats = _run(x, None, w, b, gy)
    assert stats is not None, "the statistics epilogue did not run"
    st, ntiles = stats
    assert ntiles == query("mvd_conv_stats_tiles", *sp)
    st = st.cpu().double()
    D, H, W = sp
    yd = y.double()
    t = 0
    for td in range((D + 3) // 4):
        for th in range((H + 3) // 4):
            for tw in range((W + 7) // 8):
                blk = yd[:, :, td * 4:td * 4 + 4, th * 4:th * 4 + 4, tw * 8:tw * 8 + 8]
                s1, s2 = blk.sum((2, 3, 4)), (blk * blk).sum((2, 3, 4))
                for got, want, what in ((st[:, t, :, 0], s1, "sum"), (st[:, t, :, 1], s2, "sumsq")):
                    err = (got - want).abs()
                    bar = 2e-6 * float(want.abs().max() + 1) + 2e-6 * want.abs()
                    assert bool((err <= bar).all()), f"{what} tile {t}: max abs err {float(err.max()):.3e}"
                t += 1
    assert t == ntiles
    y_plain = _plain_forward(x, w, b)
    assert torch.equal(y, y_plain), float((y - y_plain).abs().max())


def test_wino3_epilogue_deterministic():
    """Two calls give bit-identical y, dx and statistics (fixed summation order, no atomics)."""
    _skip_if_off()
    x, w, b, gy, _ = _float_case()
    y0, d0, _, s0 = _run(x, None, w, b, gy)
    y1, d1, _, s1 = _run(x, None, w, b, gy)
    assert s0 is not None and s1 is not None
    assert torch.equal(y0, y1) and torch.equal(d0, d1)
    assert torch.equal(s0[0].cpu(), s1[0].cpu())
