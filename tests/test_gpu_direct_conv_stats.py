"""InstanceNorm statistics from the epilogue of the direct fp32 conv kernels (k_fwd_mfma: the narrow-input first layer and the
chunked stride-2 form; k_fwd32s: the stride-2 kernel of the large stages): conv -> norm against fp64 with the bars of
tests/test_gpu_parity.py::test_conv_instnorm_statistics_epilogue_vs_fp64, the stand-alone statistics pass must not run
(mvd_instnorm_stats_pass_launches), and two runs are bit-identical.  The single-launch norm of small volumes is switched off
here (mvd_set_instnorm_small_max(0)): it takes its own statistics and ops would not ask the conv for them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def close(a, b, atol, rtol=0.0, what=""):
    a, b = a.detach().float().cpu(), torch.as_tensor(np.asarray(b)).float()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    assert bool((err <= tol).all()), f"{what}: max abs err {float(err.max()):.3e} (tol {atol:g}+{rtol:g}*|ref|)"


# first-layer form: ragged tiles on every axis (k_fwd_mfma<4, 1, 2>: 4 x 8 x 8 tiles, 3 x 2 x 3 of them);
# 32 -> 64 stride 2 at 10x12x18: 24 work items, the chunked kernel (unsplit for the epilogue), a partial last tile;
# 32 -> 64 stride 2 at 34x36x66: 450 work items, k_fwd32s itself (2 x 4 x 8 tiles; 17 x 18 x 33 out: ragged on every axis)
CASES = [(2, 4, 32, (9, 10, 17), 1, "k_fwd_mfma"), (2, 32, 64, (10, 12, 18), 2, "k_fwd_mfma"),
         (2, 32, 64, (34, 36, 66), 2, "k_fwd32s")]


@pytest.mark.parametrize("N,C,K,sp,stride,kernel", CASES)
def test_direct_conv_statistics_epilogue_vs_fp64(N, C, K, sp, stride, kernel):
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, i3, query
    g = torch.Generator().manual_seed(31 + C + sp[0])
    x = torch.randn(N, C, *sp, generator=g)
    w = torch.randn(K, C, 3, 3, 3, generator=g) / np.sqrt(27 * C)
    b = torch.randn(K, generator=g) * 0.1
    gamma = torch.rand(K, generator=g) + 0.5
    beta = torch.randn(K, generator=g) * 0.1
    osp = tuple((s - 1) // stride + 1 for s in sp)
    gy = torch.randn(N, K, *osp, generator=g)
    xr, wr, br, gr, ber = [t.double().requires_grad_() for t in (x, w, b, gamma, beta)]
    ref = F.leaky_relu(F.instance_norm(F.conv3d(xr, wr, br, stride, 1), None, None, gr, ber, True, 0.1, 1e-5), 0.01)
    ref.backward(gy.double())
    # tiles per sample of the kernel that runs: one wave's plane of the workgroup tile each
    tiles = query("mvd_conv3d_fwd_stats_tiles", N, *sp, C, 0, K, i3((3, 3, 3)), i3((stride,) * 3))
    od, oh, ow = osp
    if kernel == "k_fwd32s":
        assert tiles == 2 * ((od + 1) // 2) * ((oh + 3) // 4) * ((ow + 7) // 8)
    else:  # 4 x 4 MT x 8 tiles, MT = 2 or 1 (what fits the LDS beside the halo)
        assert tiles in [4 * ((od + 3) // 4) * ((oh + 4 * mt - 1) // (4 * mt)) * ((ow + 7) // 8) for mt in (1, 2)]

    def run():
        xs = [t.clone().to(DEV).requires_grad_() for t in (x, w, b, gamma, beta)]
        y = ops.Conv3dFn.apply(xs[0], None, xs[1], xs[2], (stride,) * 3)
        assert getattr(y, "_mvd_tile_stats", None) is not None, "the statistics epilogue did not run"
        assert y._mvd_tile_stats[1] == tiles
        z = ops.InstanceNormLeakyReLUFn.apply(y, xs[3], xs[4], 1e-5, 0.01)
        z.backward(gy.to(DEV))
        torch.cuda.synchronize()
        return y.detach(), z.detach(), [t.grad for t in xs]
    try:
        call("mvd_set_instnorm_small_max", 0)
        before = query("mvd_instnorm_stats_pass_launches")
        y, z, grads = run()
        assert query("mvd_instnorm_stats_pass_launches") == before, "the statistics pass over the conv output ran"
        y_b, z_b, grads_b = run()
        # the same conv output without statistics attached: the plain two-pass norm (this one runs the statistics pass)
        z2 = ops.InstanceNormLeakyReLUFn.apply(y.clone(), gamma.to(DEV), beta.to(DEV), 1e-5, 0.01)
        assert query("mvd_instnorm_stats_pass_launches") == before + 1
        saved = ops.DIRECT_CONV_STATS[0]
        ops.DIRECT_CONV_STATS[0] = False
        try:
            y_off = ops.Conv3dFn.apply(x.to(DEV), None, w.to(DEV), b.to(DEV), (stride,) * 3)
        finally:
            ops.DIRECT_CONV_STATS[0] = saved
        assert getattr(y_off, "_mvd_tile_stats", None) is None
    finally:
        call("mvd_set_instnorm_small_max", -1)
    assert torch.equal(y, y_b) and torch.equal(z, z_b), "run-to-run"
    for u, v in zip(grads, grads_b):
        assert torch.equal(u, v), "run-to-run (gradients)"
    if kernel == "k_fwd32s" or C < 16:
        assert torch.equal(y, y_off), "the epilogue changed the conv output"
    else:  # this small conv splits its reduce channels over workgroups when no epilogue is asked for: another summation order
        close(y, y_off.cpu(), 2e-5, 1e-5, "conv output, unsplit vs split")
    close(z, ref.detach(), 2e-5, 1e-5, "conv+norm output")
    close(z, z2.cpu(), 2e-6, 1e-6, "epilogue statistics vs two-pass statistics")
    close(grads[0], xr.grad, 2e-5 * float(xr.grad.abs().max()), 1e-5, "dx")
    close(grads[3], gr.grad, 2e-5 * float(gr.grad.abs().max()), 1e-5, "dgamma")
