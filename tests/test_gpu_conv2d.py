"""The 9-tap in-plane (1x3x3) conv layers -- the convs of a 2-D network and of anisotropic 3-D plans: the F(2x2,3x3) engine
k_fwd_wino2p (forward and input gradient) against fp64, against the direct engine and, on small-integer data, against
torch's fp32 result bit for bit; the weight / bias gradients of these layers through the generic weight-gradient engine;
a stride-(1,2,2) 9-tap layer through the direct engines.  The engine is forced on the small shapes with
mvd_set_wino2p_min_items(1) and restored in `finally`.

The kernel's tile is FOUR PLANES x 4 x 8 outputs over the flat (n, d) plane axis; the shapes straddle it: one whole tile,
one over in every axis (odd W), smaller than a tile, plane counts that are no multiple of 4 with D = 1 and with D > 1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS, S1 = (1, 3, 3), (1, 1, 1)


def G(a, requires_grad=False):
    t = torch.as_tensor(a).detach().to(DEV)
    if requires_grad:
        t.requires_grad_()
    return t


def close(a, b, atol, rtol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    print(f"{what}: max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})")
    assert bool((err <= atol + rtol * b.abs()).all()), f"{what}: max abs err {float(err.max()):.3e}"


def _skip_if_off():
    from multimodal_mvd_seg_amd._lib import query
    if query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0: the Winograd engines are switched off for this run")


def _run(engine, x1, x2, w, b, gy, stride=S1):
    """Conv3dFn forward + backward with the 9-tap engine forced ('wino2p') or off ('direct'); asserts that
    mvd_conv_wino2p_applicable says what runs."""
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, query, i3
    try:
        call("mvd_set_wino2p_min_items", 1 if engine == "wino2p" else 1 << 40)
        N, C1 = x1.shape[:2]
        C2 = x2.shape[1] if x2 is not None else 0
        bits = query("mvd_conv_wino2p_applicable", N, *x1.shape[2:], C1, C2, w.shape[0], i3(tuple(w.shape[2:])), i3(stride))
        assert bits == (3 if engine == "wino2p" else 0), (engine, bits)
        g1, g2 = G(x1, True), (G(x2, True) if x2 is not None else None)
        gw, gb = G(w, True), G(b, True)
        y = ops.Conv3dFn.apply(g1, g2, gw, gb, stride)
        y.backward(G(gy))
        torch.cuda.synchronize()
        return y.detach().cpu(), g1.grad.cpu(), (g2.grad.cpu() if x2 is not None else None), gw.grad.cpu(), gb.grad.cpu()
    finally:
        call("mvd_set_wino2p_min_items", -1)


# (N, C1, C2, K, D, H, W)
CASES = [
    (4, 32, 0, 32, 1, 4, 8),       # one whole tile (4 planes x 4 x 8)
    (2, 32, 0, 32, 1, 8, 16),      # 2 x 2 tiles in the plane, half a tile of planes
    (5, 32, 0, 64, 1, 5, 9),       # one over in every axis, odd W, two k-blocks
    (3, 32, 0, 64, 1, 9, 17),      # odd W, three planes
    (1, 32, 32, 32, 1, 3, 5),      # smaller than a tile, two input pointers; the dgrad writes split outputs
    (1, 32, 32, 32, 1, 5, 7),
    (2, 64, 0, 96, 3, 13, 35),     # two chunks, three k-blocks; D > 1 (anisotropic 3-D): planes must not mix
    (5, 96, 0, 32, 1, 16, 32),     # a sample count that is no multiple of 4, three chunks
]
IDS = ["x".join(str(i) for i in c) for c in CASES]


def _data(case, integer):
    N, C1, C2, K, D, H, W = case
    g = torch.Generator().manual_seed(N * 1000 + C1 + C2 + K + H * W + int(integer))
    if integer:
        ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()
        x1 = ri((N, C1, D, H, W), -2, 2)
        x2 = ri((N, C2, D, H, W), -2, 2) if C2 else None
        w, b = ri((K, C1 + C2, 1, 3, 3), -2, 2), ri((K,), -3, 3)
        gy = ri((N, K, D, H, W), -1, 1)
    else:
        x1 = torch.randn(N, C1, D, H, W, generator=g)
        x2 = torch.randn(N, C2, D, H, W, generator=g) if C2 else None
        w = torch.randn(K, C1 + C2, 1, 3, 3, generator=g) * (1.0 / np.sqrt(9 * (C1 + C2)))
        b = torch.randn(K, generator=g) * 0.1
        gy = torch.randn(N, K, D, H, W, generator=g)
    return x1, x2, w, b, gy


def _ref(x1, x2, w, b, gy, dtype, stride=S1):
    xs = [t.detach().clone().to(dtype).requires_grad_() for t in ([x1, x2] if x2 is not None else [x1])]
    wr, br = w.detach().clone().to(dtype).requires_grad_(), b.detach().clone().to(dtype).requires_grad_()
    y = F.conv3d(torch.cat(xs, 1), wr, br, stride, (0, 1, 1))
    y.backward(gy.to(dtype))
    return y.detach(), xs[0].grad, (xs[1].grad if x2 is not None else None), wr.grad, br.grad


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wino2p_fwd_dgrad_vs_fp64_and_direct(case):
    """Bars: 1e-5 absolute + 1e-5 relative, those of test_conv3d_winograd_engine_vs_torch_fp64 for the same transform."""
    _skip_if_off()
    x1, x2, w, b, gy = _data(case, False)
    ry, r1, r2, _, _ = _ref(x1, x2, w, b, gy, torch.float64)
    y, d1, d2, _, _ = _run("wino2p", x1, x2, w, b, gy)
    close(y, ry, 1e-5, 1e-5, "y vs fp64")
    close(d1, r1, 1e-5, 1e-5, "dx1 vs fp64")
    if x2 is not None:
        close(d2, r2, 1e-5, 1e-5, "dx2 vs fp64")
    yd, dd1, dd2, _, _ = _run("direct", x1, x2, w, b, gy)
    close(y, yd, 1e-5, 1e-5, "y vs direct engine")
    close(d1, dd1, 1e-5, 1e-5, "dx1 vs direct engine")
    if x2 is not None:
        close(d2, dd2, 1e-5, 1e-5, "dx2 vs direct engine")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wino2p_exact_integer_data(case):
    """x, w in -2..2: U = G g G^T is a multiple of 1/4 with |U| <= 9, |V| <= 8; at the 96 reduce channels of the largest case
    every partial sum stays below 96 * 36 * 8 quarters < 2^24, so the kernel is exact and equals torch's fp32 result bit
    for bit (the discipline of test_cfg2_conv_exact_integer_data)."""
    _skip_if_off()
    x1, x2, w, b, gy = _data(case, True)
    ry, r1, r2, _, _ = _ref(x1, x2, w, b, gy, torch.float32)
    y, d1, d2, _, _ = _run("wino2p", x1, x2, w, b, gy)
    assert torch.equal(y, ry), float((y - ry).abs().max())
    assert torch.equal(d1, r1), float((d1 - r1).abs().max())
    if x2 is not None:
        assert torch.equal(d2, r2), float((d2 - r2).abs().max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_1x3x3_wgrad_vs_fp64_and_exact(case):
    """Weight and bias gradients of (1,3,3) layers through the generic weight-gradient engine (no Winograd form for 9 taps):
    bars of test_conv3d_engine_shapes_vs_torch_fp64; bit-exact on integer data.  Passes without the new kernel: nothing
    covered these shapes."""
    x1, x2, w, b, gy = _data(case, False)
    _, _, _, rw, rb = _ref(x1, x2, w, b, gy, torch.float64)
    _, _, _, dw, db = _run("direct", x1, x2, w, b, gy)
    close(dw, rw, 2e-5 * float(rw.abs().max()), 1e-5, "dw")
    close(db, rb, 1e-4, 1e-5, "db")
    x1, x2, w, b, gy = _data(case, True)
    _, _, _, rw, rb = _ref(x1, x2, w, b, gy, torch.float32)
    _, _, _, dw, db = _run("direct", x1, x2, w, b, gy)
    assert torch.equal(dw, rw), float((dw - rw).abs().max())
    assert torch.equal(db, rb), float((db - rb).abs().max())


@pytest.mark.parametrize("N,C,K,D,H,W", [(2, 32, 64, 1, 9, 14), (1, 64, 64, 3, 8, 11)])
def test_1x3x3_stride122_direct_engine(N, C, K, D, H, W):
    """A stride-(1,2,2) 9-tap layer (the down-sampling conv of a 2-D stage): forward, dgrad, wgrad through the direct
    engines against fp64 (bars of test_conv3d_engine_shapes_vs_torch_fp64) and bit-exact on integer data."""
    st = (1, 2, 2)
    g = torch.Generator().manual_seed(N + C + K + H)
    x = torch.randn(N, C, D, H, W, generator=g)
    w = torch.randn(K, C, 1, 3, 3, generator=g) / np.sqrt(9 * C)
    b = torch.randn(K, generator=g) * 0.1
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, K, D, oh, ow, generator=g)
    ry, r1, _, rw, rb = _ref(x, None, w, b, gy, torch.float64, st)
    y, d1, _, dw, db = _run("direct", x, None, w, b, gy, st)
    close(y, ry, 2e-5, 1e-5, "y")
    close(d1, r1, 2e-5, 1e-5, "dx")
    close(dw, rw, 2e-5 * float(rw.abs().max()), 1e-5, "dw")
    close(db, rb, 1e-4, 1e-5, "db")
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()
    x, w, b, gy = ri(x.shape, -2, 2), ri(w.shape, -2, 2), ri(b.shape, -3, 3), ri(gy.shape, -1, 1)
    ry, r1, _, rw, rb = _ref(x, None, w, b, gy, torch.float32, st)
    y, d1, _, dw, db = _run("direct", x, None, w, b, gy, st)
    assert torch.equal(y, ry) and torch.equal(d1, r1) and torch.equal(dw, rw) and torch.equal(db, rb)


def test_wino2p_only_kernel_size_133_qualifies():
    """Other 9-tap kernels, e.g. (3,3,1), keep the direct engine; so do stride-2 and narrow-input layers."""
    from multimodal_mvd_seg_amd._lib import call, query, i3
    try:
        call("mvd_set_wino2p_min_items", 1)
        assert query("mvd_conv_wino2p_applicable", 2, 4, 16, 16, 32, 0, 32, i3((1, 3, 3)), i3((1, 1, 1))) == 3
        for ks, st, c in (((3, 3, 1), (1, 1, 1), 32), ((3, 1, 3), (1, 1, 1), 32), ((3, 3, 3), (1, 1, 1), 32),
                          ((1, 3, 3), (1, 2, 2), 32), ((1, 3, 3), (1, 1, 1), 4)):
            assert query("mvd_conv_wino2p_applicable", 2, 4, 16, 16, c, 0, 32, i3(ks), i3(st)) == 0, (ks, st, c)
        call("mvd_set_wino2p_min_items", 1 << 40)
        assert query("mvd_conv_wino2p_applicable", 2, 4, 16, 16, 32, 0, 32, i3((1, 3, 3)), i3((1, 1, 1))) == 0
    finally:
        call("mvd_set_wino2p_min_items", -1)
    # a (3,3,1) layer computes the right thing on the direct engine with the 9-tap engine forced on
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 32, 6, 7, 5, generator=g)
    w = torch.randn(32, 32, 3, 3, 1, generator=g) / np.sqrt(9 * 32)
    from multimodal_mvd_seg_amd import ops
    try:
        call("mvd_set_wino2p_min_items", 1)
        y = ops.Conv3dFn.apply(G(x), None, G(w), None, (1, 1, 1))
    finally:
        call("mvd_set_wino2p_min_items", -1)
    close(y, F.conv3d(x.double(), w.double(), None, 1, (1, 1, 0)), 2e-5, 1e-5, "(3,3,1) layer")


def test_wino2p_batched_pack_equals_per_layer_pack():
    """The T = 9 job form of the one-launch repack writes the tables mvd_pack_weight_wino2p writes, bit for bit."""
    import ctypes
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, query
    K, C = 64, 96
    w = G(torch.randn(K, C, 1, 3, 3, generator=torch.Generator().manual_seed(3)))
    n = query("mvd_wino2p_weight_elems", C, K)
    assert n == 16 * C * K
    one = [torch.zeros(n, device=DEV) for _ in range(2)]
    call("mvd_pack_weight_wino2p", w.data_ptr(), one[0].data_ptr(), one[1].data_ptr(), K, C, ops._stream())
    wf, wb = torch.empty(9 * C * K, device=DEV), torch.empty(9 * C * K, device=DEV)
    bat = [torch.zeros(n, device=DEV) for _ in range(2)]
    PA, IA = ctypes.c_void_p * 1, ctypes.c_int * 1
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    call("mvd_pack_weights_batch3", 1, cast(PA(w.data_ptr())), cast(PA(wf.data_ptr())), cast(PA(wb.data_ptr())),
         cast(PA(bat[0].data_ptr())), cast(PA(bat[1].data_ptr())), cast(PA(None)), cast(PA(None)), cast(IA(K)), cast(IA(C)),
         cast(IA(9)), cast(IA(0)), ops._stream())
    torch.cuda.synchronize()
    rf, rb = ops.pack_weight(w, False)
    assert torch.equal(one[0], bat[0]) and torch.equal(one[1], bat[1])
    assert torch.equal(wf, rf.flatten()) and torch.equal(wb, rb.flatten())
    assert float(one[0].abs().sum()) > 0 and float(one[1].abs().sum()) > 0
