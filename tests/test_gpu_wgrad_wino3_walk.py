"""The tile walk of k_wgrad_wino3: a split's loop over several tiles across samples, the double-buffered LDS
images, the wave -> (pz, a) mapping and the empty descriptors past the last tile, through mvd_conv3d_wgrad.

x and dy are integers in {-2..2}: |V| <= 16 and |E| <= 16 per position, a split walks at most 6 tiles of 16 octets, so a
partial is at most 6 x 16 x 256 = 24576 < 2^24 in magnitude: every fp32 partial is an exact integer, the fp64 reduce is
exact (G^T entries are multiples of 1/8) and dW / db must EQUAL the fp64 reference.  The engine is forced with
mvd_set_wgrad_wino3_min_items (restored in `finally`) and mvd_wgrad_wino3_launches proves the 3-D kernel ran."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS, ST = (3, 3, 3), (1, 1, 1)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _wgrad_wino3(x1, x2, dy):
    from multimodal_mvd_seg_amd._lib import call, i3, query
    N, D, H, W, C1 = x1.shape
    C2 = x2.shape[-1] if x2 is not None else 0
    K = dy.shape[-1]
    try:
        call("mvd_set_wgrad_wino3_min_items", 1)
        assert query("mvd_conv_wgrad_wino3_applicable", N, D, H, W, C1, C2, K, i3(KS), i3(ST)) == 1
        nbytes = query("mvd_conv3d_wgrad_workspace_bytes", C1 + C2, K, 27, N, D, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        dw = torch.empty(K, C1 + C2, 27, dtype=torch.float32, device=DEV)
        db = torch.empty(K, dtype=torch.float32, device=DEV)
        before = query("mvd_wgrad_wino3_launches")
        call("mvd_conv3d_wgrad", _p(x1), C1, _p(x2), C2, _p(dy), _p(dw), _p(db), N, D, H, W, K, i3(KS), i3(ST),
             _p(ws), ctypes.c_size_t(nbytes), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert query("mvd_wgrad_wino3_launches") - before == 1
        return dw.cpu(), db.cpu()
    finally:
        call("mvd_set_wgrad_wino3_min_items", -1)


def _ref64(x1, x2, dy):
    x = torch.cat([x1, x2], -1) if x2 is not None else x1
    xc = x.double().cpu().permute(0, 4, 1, 2, 3)
    gc = dy.double().cpu().permute(0, 4, 1, 2, 3)
    K, C = gc.shape[1], xc.shape[1]
    dw = torch.nn.grad.conv3d_weight(xc, (K, C, 3, 3, 3), gc, stride=1, padding=1)
    return dw.reshape(K, C, 27), gc.sum((0, 2, 3, 4))


def _setup():
    from multimodal_mvd_seg_amd import _lib
    _lib.load()
    if _lib.query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0 for this run")


def _data(shape, rng, integer):
    if integer:
        return torch.from_numpy(rng.integers(-2, 3, size=shape).astype(np.float32)).to(DEV)
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV)


# (5, 9, 11) = 3 x 2 x 2 tiles per sample with a ragged last tile on every axis; (3, 11, 6) = 2 x 2 x 1 tiles
@pytest.mark.parametrize("N,sp,C1,C2,K", [
    (2, (5, 9, 11), 256, 0, 256),    # 4 splits x 6 tiles (even), both samples
    (3, (5, 9, 11), 128, 128, 128),  # 8 splits x 4 or 5 tiles (odd too), two pointers, the channel block crosses them
    (1, (3, 11, 6), 64, 0, 96),      # 4 tiles < 42 splits: one trip, the descriptors past the last tile are empty
])
def test_walk_exact_integer(N, sp, C1, C2, K):
    _setup()
    rng = np.random.default_rng(N + C1 + K)
    x1 = _data((N, *sp, C1), rng, True)
    x2 = _data((N, *sp, C2), rng, True) if C2 else None
    dy = _data((N, *sp, K), rng, True)
    dw, db = _wgrad_wino3(x1, x2, dy)
    rw, rb = _ref64(x1, x2, dy)
    assert torch.equal(dw.double(), rw), float((dw.double() - rw).abs().max())
    assert torch.equal(db.double(), rb), float((db.double() - rb).abs().max())


def test_walk_normal_data_bit_identical_and_fp64_parity():
    _setup()
    N, sp, C, K = 2, (5, 9, 11), 256, 256
    rng = np.random.default_rng(11)
    x1, dy = _data((N, *sp, C), rng, False), _data((N, *sp, K), rng, False)
    dw, db = _wgrad_wino3(x1, None, dy)
    dw2, db2 = _wgrad_wino3(x1, None, dy)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    rw, rb = _ref64(x1, None, dy)
    scale = float(rw.abs().max())
    err = float((dw.double() - rw).abs().max())
    # the bar of test_wgrad_wino3_fp64_parity
    assert err <= 1e-5 * max(scale, 1.0) + 1e-5 * float(np.sqrt(N * np.prod(sp))), (err, scale)
    assert float((db.double() - rb).abs().max()) <= 1e-5 * max(float(rb.abs().max()), 1.0)
