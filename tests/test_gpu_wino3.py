"""The F(2x2x2,3x3x3) Winograd engine (k_fwd_wino3): forward and input gradient against fp64 and against the direct
and F(2x2,3x3) engines, exact-integer parity, the statistics epilogue, the packed tables and run-to-run determinism.
The 3-D engine is forced on small shapes with mvd_set_wino3_min_items and restored in `finally`."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def G(a, requires_grad=False):
    t = torch.as_tensor(a).to(DEV)
    if requires_grad:
        t.requires_grad_()
    return t


def close(a, b, atol, rtol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), f"{what}: max abs err {float(err.max()):.3e}"


def _engine(name):
    """(wino min items, wino3 min items) that select one engine for a small problem"""
    return {"wino3": (1, 1), "wino2": (1, 1 << 40), "direct": (1 << 40, 1 << 40)}[name]


def _run(engine, x1, x2, w, b, gy):
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, query, i3
    m2, m3 = _engine(engine)
    try:
        call("mvd_set_wino_min_items", m2)
        call("mvd_set_wino3_min_items", m3)
        N, C1 = x1.shape[:2]
        C2 = x2.shape[1] if x2 is not None else 0
        K = w.shape[0]
        sp = tuple(x1.shape[2:])
        bits3 = query("mvd_conv_wino3_applicable", N, *sp, C1, C2, K, i3((3, 3, 3)), i3((1, 1, 1)))
        assert bits3 == (3 if engine == "wino3" else 0), (engine, bits3)
        g1, g2 = G(x1, True), (G(x2, True) if x2 is not None else None)
        y = ops.Conv3dFn.apply(g1, g2, G(w, True), G(b, True), (1, 1, 1))
        stats = getattr(y, "_mvd_tile_stats", None)
        y.backward(G(gy))
        torch.cuda.synchronize()
        return y.detach().cpu(), g1.grad.cpu(), (g2.grad.cpu() if x2 is not None else None), stats
    finally:
        call("mvd_set_wino_min_items", -1)
        call("mvd_set_wino3_min_items", -1)


def _skip_if_off():
    from multimodal_mvd_seg_amd._lib import query, i3
    if query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0: the Winograd engines are switched off for this run")
    try:
        from multimodal_mvd_seg_amd._lib import call
        call("mvd_set_wino_min_items", 1)
        call("mvd_set_wino3_min_items", 1)
        if not query("mvd_conv_wino3_applicable", 1, 8, 8, 8, 32, 0, 32, i3((3, 3, 3)), i3((1, 1, 1))):
            pytest.skip("MVD_WINO3=0: the 3-D engine is switched off for this run")
    finally:
        call("mvd_set_wino_min_items", -1)
        call("mvd_set_wino3_min_items", -1)


# (C1, C2, K, spatial, N): whole tiles; ragged D / H / W; two input pointers and split dgrad outputs; several chunks and
# k-blocks; N = 2
CASES = [
    (32, 0, 32, (8, 8, 8), 1),
    (32, 0, 32, (9, 11, 13), 1),
    (32, 32, 64, (6, 10, 7), 2),
    (64, 0, 96, (5, 9, 17), 1),
    (96, 32, 32, (4, 8, 8), 2),
]


@pytest.mark.parametrize("C1,C2,K,sp,N", CASES)
def test_wino3_fwd_dgrad_vs_fp64_direct_and_wino2(C1, C2, K, sp, N):
    _skip_if_off()
    g = torch.Generator().manual_seed(C1 * 7 + C2 + K + sp[2])
    x1 = torch.randn(N, C1, *sp, generator=g)
    x2 = torch.randn(N, C2, *sp, generator=g) if C2 else None
    w = torch.randn(K, C1 + C2, 3, 3, 3, generator=g) * (1.0 / np.sqrt(27 * (C1 + C2)))
    b = torch.randn(K, generator=g) * 0.1
    xs = [t.double().requires_grad_() for t in ([x1, x2] if C2 else [x1])]
    ref = F.conv3d(torch.cat(xs, 1), w.double(), b.double(), 1, 1)
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(gy)
    out = {e: _run(e, x1, x2, w, b, gy.float()) for e in ("wino3", "wino2", "direct")}
    y, d1, d2, _ = out["wino3"]
    scale = float(ref.detach().abs().max())
    close(y, ref, 1e-5 * scale, 1e-5, "y vs fp64")
    close(d1, xs[0].grad, 1e-5 * float(xs[0].grad.abs().max()), 1e-5, "dx1 vs fp64")
    if C2:
        close(d2, xs[1].grad, 1e-5 * float(xs[1].grad.abs().max()), 1e-5, "dx2 vs fp64")
    for other in ("wino2", "direct"):
        close(y, out[other][0], 1e-5 * scale, 1e-5, f"y vs {other}")
        close(d1, out[other][1], 1e-5 * float(d1.abs().max()), 1e-5, f"dx1 vs {other}")


@pytest.mark.parametrize("C,K,sp", [(32, 32, (6, 9, 11)), (64, 32, (5, 8, 7)), (512, 32, (4, 8, 8))])
def test_wino3_exact_integer_data(C, K, sp):
    """Small-integer activations and weights: with |w| <= 1, U is a multiple of 1/8 with |U| <= (3/2)^3; with |x| <= 2,
    |V| <= 8 * 2.  At 512 reduce channels every partial sum stays below 512 * 16 * 3.375 * 8 = 221184 eighths < 2^24:
    the 3-D kernel is exact and its output equals torch's bit for bit."""
    _skip_if_off()
    g = torch.Generator().manual_seed(C + K)
    x = torch.randint(-2, 3, (1, C, *sp), generator=g).float()
    w = torch.randint(-1, 2, (K, C, 3, 3, 3), generator=g).float()
    b = torch.randint(-4, 5, (K,), generator=g).float()
    ref = F.conv3d(x.double(), w.double(), b.double(), 1, 1)
    gy = torch.randint(-2, 3, ref.shape, generator=g).float()
    refx = torch.nn.grad.conv3d_input(x.shape, w.double(), gy.double(), 1, 1)
    y, d1, _, _ = _run("wino3", x, None, w, b, gy)
    assert torch.equal(y.double(), ref), float((y.double() - ref).abs().max())
    assert torch.equal(d1.double(), refx), float((d1.double() - refx).abs().max())


def test_wino3_statistics_epilogue():
    """Per-tile (sum, sum of squares) in the 4x4x8-tile layout of mvd_conv_stats_tiles, ragged H so that the second
    4-row half of the last 8-row tile does not exist, against statistics taken from the output itself."""
    _skip_if_off()
    from multimodal_mvd_seg_amd._lib import query
    g = torch.Generator().manual_seed(5)
    N, C, K, sp = 2, 32, 64, (7, 12, 13)
    x = torch.randn(N, C, *sp, generator=g)
    w = torch.randn(K, C, 3, 3, 3, generator=g) / np.sqrt(27 * C)
    b = torch.randn(K, generator=g) * 0.1
    gy = torch.randn(N, K, *sp, generator=g)
    y, _, _, stats = _run("wino3", x, None, w, b, gy)
    assert stats is not None, "the statistics epilogue did not run"
    st, ntiles = stats
    assert ntiles == query("mvd_conv_stats_tiles", *sp)
    st = st.cpu().double()
    D, H, W = sp
    nth, ntw = (H + 3) // 4, (W + 7) // 8
    yd = y.double()
    t = 0
    for td in range((D + 3) // 4):
        for th in range(nth):
            for tw in range(ntw):
                blk = yd[:, :, td * 4:td * 4 + 4, th * 4:th * 4 + 4, tw * 8:tw * 8 + 8]
                s1, s2 = blk.sum((2, 3, 4)), (blk * blk).sum((2, 3, 4))
                close(st[:, t, :, 0], s1, 2e-6 * float(s1.abs().max() + 1), 2e-6, f"sum tile {t}")
                close(st[:, t, :, 1], s2, 2e-6 * float(s2.abs().max() + 1), 2e-6, f"sumsq tile {t}")
                t += 1
    assert t == ntiles


def test_wino3_batched_pack_equals_per_layer_pack():
    _skip_if_off()
    from multimodal_mvd_seg_amd._lib import call, query
    g = torch.Generator().manual_seed(3)
    shapes = [(32, 32), (64, 32), (32, 96)]
    ws = [G(torch.randn(K, C, 3, 3, 3, generator=g)) for K, C in shapes]
    n = len(ws)
    s = torch.cuda.current_stream().cuda_stream
    PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
    mk = lambda K, C, m: torch.zeros(m, device=DEV)
    wf = [mk(K, C, 27 * C * K) for K, C in shapes]
    wb = [mk(K, C, 27 * C * K) for K, C in shapes]
    vf = [mk(K, C, query("mvd_wino3_weight_elems", C, K)) for K, C in shapes]
    vb = [mk(K, C, query("mvd_wino3_weight_elems", C, K)) for K, C in shapes]
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    ptrs = lambda ts: cast(PA(*[t.data_ptr() for t in ts]))
    nul = cast(PA(*([None] * n)))
    call("mvd_pack_weights_batch3", n, ptrs(ws), ptrs(wf), ptrs(wb), nul, nul, ptrs(vf), ptrs(vb),
         cast(IA(*[K for K, _ in shapes])), cast(IA(*[C for _, C in shapes])), cast(IA(*([27] * n))), cast(IA(*([0] * n))), s)
    for (K, C), w, f, bb in zip(shapes, ws, vf, vb):
        rf, rb = torch.zeros_like(f), torch.zeros_like(bb)
        call("mvd_pack_weight_wino3", w.data_ptr(), rf.data_ptr(), rb.data_ptr(), K, C, s)
        torch.cuda.synchronize()
        assert torch.equal(f, rf) and torch.equal(bb, rb), (K, C)


def test_wino3_pack_cache_follows_optimizer_step():
    """The conv's cached 3-D tables are re-packed by repack_all after an in-place update of the weight."""
    _skip_if_off()
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, query
    g = torch.Generator().manual_seed(4)
    x = G(torch.randn(1, 32, 8, 8, 8, generator=g))
    w = G(torch.randn(32, 32, 3, 3, 3, generator=g) * 0.05, True)
    b = G(torch.zeros(32), True)
    try:
        call("mvd_set_wino_min_items", 1)
        call("mvd_set_wino3_min_items", 1)
        ops.Conv3dFn.apply(x, None, w, b, (1, 1, 1))
        e = w._mvd_pack
        assert e.vf is not None
        with torch.no_grad():
            w.mul_(0.5)
        ops.repack_all()
        ref = torch.empty_like(e.vf)
        call("mvd_pack_weight_wino3", w.data_ptr(), ref.data_ptr(), None, 32, 32, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(e.vf, ref)
        y = ops.Conv3dFn.apply(x, None, w, b, (1, 1, 1))
        refy = F.conv3d(x.double().cpu(), w.detach().double().cpu(), None, 1, 1)
        close(y, refy, 1e-5 * float(refy.abs().max()), 1e-5, "y after the update")
    finally:
        call("mvd_set_wino_min_items", -1)
        call("mvd_set_wino3_min_items", -1)


def test_wino3_deterministic():
    _skip_if_off()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 64, 9, 10, 11, generator=g)
    w = torch.randn(32, 64, 3, 3, 3, generator=g) * 0.03
    b = torch.randn(32, generator=g)
    gy = torch.randn(2, 32, 9, 10, 11, generator=g)
    r1 = _run("wino3", x, None, w, b, gy)
    r2 = _run("wino3", x, None, w, b, gy)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    assert torch.equal(r1[3][0], r2[3][0])
