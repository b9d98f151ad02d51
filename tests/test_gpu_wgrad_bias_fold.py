"""Bias gradient inside the fp32 weight-gradient kernels that used to leave it to a column-sum pass over dy: the narrow-input
kernel (k_wgrad_smallc, a ones operand in an idle GEMM row) and the transposed convs (k_wgrad_mfma with one A slot for all
taps: each wave sums the dy fragments it stages).  The conv has no norm behind it, so the reference bias gradient is a plain
sum, not round-off about zero.  Bars, those tests/test_gpu_cfg2.py applies to dbias for these kernels: the conv weight
gradients max|db - db64| <= 2e-6 * max_k sum|dy| + 1e-12 (test_cfg2_conv_block_vs_fp64), the transposed ones 1e-5 relative L2
(test_cfg2_convT_block_vs_fp64); dw bit-identical with the fold on and off."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
D64 = torch.float64
CL = torch.channels_last_3d


def rel_l2(a, ref):
    a, ref = a.detach().cpu().to(D64), ref.detach().cpu().to(D64)
    assert a.shape == ref.shape, (tuple(a.shape), tuple(ref.shape))
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def _grads(ops, kind, x, w, b, gy, stride, fold):
    from multimodal_mvd_seg_amd._lib import call
    call("mvd_set_wgrad_bias_fold", int(fold))
    try:
        xx, ww, bb = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        if kind == "conv":
            y = ops.Conv3dFn.apply(xx, None, ww, bb, stride)
        else:
            y = ops.ConvTranspose3dFn.apply(xx, ww, bb, stride)
        y.backward(gy)
        torch.cuda.synchronize()
    finally:
        call("mvd_set_wgrad_bias_fold", -1)
    return ww.grad, bb.grad


# conv 4 -> 32 at 9x10x17: the narrow-input kernel, ragged tiles on every axis; conv 32 -> 64 stride 2 at 10x12x18: the
# generic kernel (its bias rows predate this file: the fold switch must leave it alone); transposed 64 -> 32 stride 2 (8 taps, two
# per wave) ragged, and stride (1, 2, 2) (4 taps, one per wave); 320 -> 320: ten channel blocks, only the first sums
CASES = [("conv", 2, 4, 32, (9, 10, 17), (1, 1, 1)), ("conv", 2, 32, 64, (10, 12, 18), (2, 2, 2)),
         ("convT", 2, 64, 32, (5, 6, 9), (2, 2, 2)), ("convT", 1, 64, 32, (4, 6, 5), (1, 2, 2)),
         ("convT", 2, 320, 320, (2, 2, 2), (2, 2, 2))]


@pytest.mark.parametrize("kind,N,C,K,sp,stride", CASES)
def test_bias_gradient_inside_the_weight_gradient_kernels(kind, N, C, K, sp, stride):
    from multimodal_mvd_seg_amd import ops
    g = torch.Generator().manual_seed(C + K + sp[2])
    x = torch.randn(N, C, *sp, generator=g).to(DEV).contiguous(memory_format=CL)
    if kind == "conv":
        w = (torch.randn(K, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5).to(DEV)
        osp = tuple((s - 1) // st + 1 for s, st in zip(sp, stride))
    else:
        w = (torch.randn(C, K, *stride, generator=g) / C ** 0.5).to(DEV)
        osp = tuple(s * st for s, st in zip(sp, stride))
    b = (torch.randn(K, generator=g) * 0.1).to(DEV)
    gy = (torch.randn(N, K, *osp, generator=g) + 0.25).to(DEV).contiguous(memory_format=CL)
    dw_on, db_on = _grads(ops, kind, x, w, b, gy, stride, True)
    dw_off, db_off = _grads(ops, kind, x, w, b, gy, stride, False)
    assert torch.equal(dw_on, dw_off), f"dw moved: {int((dw_on != dw_off).sum())} of {dw_on.numel()} values"
    dw2, db2 = _grads(ops, kind, x, w, b, gy, stride, True)
    assert torch.equal(dw_on, dw2) and torch.equal(db_on, db2), "run-to-run"
    x64, w64, gy64 = x.cpu().to(D64), w.cpu().to(D64).requires_grad_(), gy.cpu().to(D64)
    b64 = b.cpu().to(D64).requires_grad_()
    y64 = F.conv3d(x64, w64, b64, stride, 1) if kind == "conv" else F.conv_transpose3d(x64, w64, b64, stride)
    y64.backward(gy64)
    e_on, e_off, e_w = rel_l2(db_on, b64.grad), rel_l2(db_off, b64.grad), rel_l2(dw_on, w64.grad)
    a_on = float((db_on.cpu().to(D64) - b64.grad).abs().max())
    a_off = float((db_off.cpu().to(D64) - b64.grad).abs().max())
    db_tol = 2e-6 * float(gy64.abs().sum((0, 2, 3, 4)).max()) + 1e-12
    print(f"[{kind} {C}->{K} {sp} s{stride}] db fold {e_on:.1e} (max abs {a_on:.1e}) column sums {e_off:.1e} (max abs {a_off:.1e}) "
          f"abs bound {db_tol:.1e} dw {e_w:.1e}")
    if kind == "conv":
        assert a_on <= db_tol and a_off <= db_tol, f"db max abs error vs fp64: fold {a_on:.2e}, column sums {a_off:.2e} > {db_tol:.2e}"
    else:
        assert e_on <= 1e-5 and e_off <= 1e-5, f"db relative L2 error vs fp64: fold {e_on:.2e}, column sums {e_off:.2e}"
    assert e_w <= 1e-5, f"dw relative L2 error vs fp64 {e_w:.2e}"
