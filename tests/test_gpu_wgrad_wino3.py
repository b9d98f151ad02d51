"""The F(2x2x2,3x3x3) weight-gradient kernel (k_wgrad_wino3 + k_wgrad_reduce_wino3) through mvd_conv3d_wgrad: dW and db
against fp64 torch at small, odd and ragged shapes (two-pointer input included), exact-integer agreement with the
F(2x2,3x3) kernel at every stride-1 fp32 layer of configs[1], run-to-run bit-identity, and proof
that the 3-D kernel ran (a workspace fallback would not).  The engine is forced with mvd_set_wgrad_wino3_min_items and
restored in `finally`."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS, ST = (3, 3, 3), (1, 1, 1)

# stride-1 fp32 3x3x3 layers of configs[1] (batch 2): (size, C1, C2, K)
CFG1_LAYERS = [(128, 32, 0, 32), (128, 32, 32, 32), (64, 64, 0, 64), (64, 64, 64, 64), (32, 128, 0, 128),
               (32, 128, 128, 128), (16, 256, 0, 256), (16, 256, 256, 256)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _wgrad(engine, x1, x2, dy):
    """dW [K][C][27] and db [K] of NDHWC fp32 x1 / x2 / dy; engine: 'wino3' or 'wino2' (F(2x2,3x3))"""
    from multimodal_mvd_seg_amd._lib import call, i3, query
    N, D, H, W, C1 = x1.shape
    C2 = x2.shape[-1] if x2 is not None else 0
    K = dy.shape[-1]
    try:
        call("mvd_set_wgrad_wino3_min_items", 1 if engine == "wino3" else 1 << 40)
        applic = query("mvd_conv_wgrad_wino3_applicable", N, D, H, W, C1, C2, K, i3(KS), i3(ST))
        assert applic == (1 if engine == "wino3" else 0), (engine, applic)
        nbytes = query("mvd_conv3d_wgrad_workspace_bytes", C1 + C2, K, 27, N, D, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        dw = torch.empty(K, C1 + C2, 27, dtype=torch.float32, device=DEV)
        db = torch.empty(K, dtype=torch.float32, device=DEV)
        before = query("mvd_wgrad_wino3_launches")
        call("mvd_conv3d_wgrad", _p(x1), C1, _p(x2), C2, _p(dy), _p(dw), _p(db), N, D, H, W, K, i3(KS), i3(ST),
             _p(ws), ctypes.c_size_t(nbytes), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        ran = query("mvd_wgrad_wino3_launches") - before
        assert ran == (1 if engine == "wino3" else 0), (engine, ran)
        return dw.cpu(), db.cpu()
    finally:
        call("mvd_set_wgrad_wino3_min_items", -1)


def _torch_ref(x1, x2, dy):
    x = torch.cat([x1, x2], -1) if x2 is not None else x1
    xc = x.double().cpu().permute(0, 4, 1, 2, 3)
    gc = dy.double().cpu().permute(0, 4, 1, 2, 3)
    K, C = gc.shape[1], xc.shape[1]
    dw = torch.nn.grad.conv3d_weight(xc, (K, C, 3, 3, 3), gc, stride=1, padding=1)
    return dw.reshape(K, C, 27), gc.sum((0, 2, 3, 4))


def _skip_if_off():
    from multimodal_mvd_seg_amd._lib import query
    if query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0 for this run")


def _data(shape, rng, integer=False):
    if integer:
        return torch.from_numpy(rng.integers(-2, 3, size=shape).astype(np.float32)).to(DEV)
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("N,sp,C1,C2,K", [
    (1, (8, 8, 8), 32, 0, 32),
    (2, (5, 7, 9), 32, 0, 64),      # odd, ragged in every axis
    (1, (3, 11, 6), 64, 0, 32),     # fewer planes than a tile, ragged rows
    (2, (6, 9, 10), 32, 32, 32),    # two-pointer (concatenated skip) input
    (1, (4, 16, 17), 64, 32, 64),
])
def test_wgrad_wino3_fp64_parity(N, sp, C1, C2, K):
    from multimodal_mvd_seg_amd import _lib
    _lib.load()
    _skip_if_off()
    rng = np.random.default_rng(7)
    x1 = _data((N, *sp, C1), rng)
    x2 = _data((N, *sp, C2), rng) if C2 else None
    dy = _data((N, *sp, K), rng)
    dw, db = _wgrad("wino3", x1, x2, dy)
    rw, rb = _torch_ref(x1, x2, dy)
    scale = float(rw.abs().max())
    err = float((dw.double() - rw).abs().max())
    assert err <= 1e-5 * max(scale, 1.0) + 1e-5 * float(np.sqrt(N * np.prod(sp))), (err, scale)
    assert float((db.double() - rb).abs().max()) <= 1e-5 * max(float(rb.abs().max()), 1.0)


def test_wgrad_wino3_deterministic():
    from multimodal_mvd_seg_amd import _lib
    _lib.load()
    _skip_if_off()
    rng = np.random.default_rng(3)
    x1, x2, dy = _data((2, 12, 20, 18, 32), rng), _data((2, 12, 20, 18, 32), rng), _data((2, 12, 20, 18, 64), rng)
    a = _wgrad("wino3", x1, x2, dy)
    b = _wgrad("wino3", x1, x2, dy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("S,C1,C2,K", CFG1_LAYERS)
def test_wgrad_wino3_cfg1_exact_integer(S, C1, C2, K):
    """x in {-2..2}, dy in {-2..2}: |V| <= 8 * 2 = 16 and |E| <= 8 * 2 per position, so a split's partial is at most
    octets per split x 16 x 16.  With the split count of one workgroup per CU (256 / (C/32 * K/32) splits, at least 1)
    a layer has at most N * S^3 / 8 * (C/32) * (K/32) / 256 octets per split: 4096 at batch 2 (128^3, 32+32 -> 32),
    4096 x 256 = 2^20 < 2^24, so every fp32 partial is an exact integer, the fp64 reduce is exact (G^T entries are
    multiples of 1/8) and dW must equal the F(2x2,3x3) kernel's (also exact) bit for bit.  The launch counter proves the 3-D kernel ran at the shape."""
    from multimodal_mvd_seg_amd import _lib
    _lib.load()
    _skip_if_off()
    rng = np.random.default_rng(S + C1 + C2)
    N = 2
    x1 = _data((N, S, S, S, C1), rng, True)
    x2 = _data((N, S, S, S, C2), rng, True) if C2 else None
    dy = _data((N, S, S, S, K), rng, True)
    # the default selection does not depend on the batch
    from multimodal_mvd_seg_amd._lib import i3, query
    assert (query("mvd_conv_wgrad_wino3_applicable", N, S, S, S, C1, C2, K, i3(KS), i3(ST)) ==
            query("mvd_conv_wgrad_wino3_applicable", 1, S, S, S, C1, C2, K, i3(KS), i3(ST)))
    d3, b3 = _wgrad("wino3", x1, x2, dy)
    d2, b2 = _wgrad("wino2", x1, x2, dy)
    assert torch.equal(d3, d2), float((d3 - d2).abs().max())
    assert torch.equal(b3, b2)
    assert bool((d3 == d3.round()).all())
