"""The single-launch InstanceNorm + LeakyReLU of small volumes (k_in_small_fwd / k_in_small_bwd: a workgroup keeps 16
channels of a sample in registers) against the fp64 oracle, with the parametrisation and bars of
tests/test_gpu_parity.py::test_instnorm_lrelu_small_volumes_vs_fp64 (y 2e-6, dx 5e-6 * max, dgamma / dbeta 1e-5 * max),
which path ran (mvd_instnorm_single_launches), the limit itself, and run-to-run equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
D64 = torch.float64


def _run(ops, x, gamma, beta, dy):
    xx, g, b = (t.clone().requires_grad_() for t in (x, gamma, beta))
    y = ops.InstanceNormLeakyReLUFn.apply(xx, g, b, 1e-5, 0.01)
    y.backward(dy)
    torch.cuda.synchronize()
    return [y.detach(), xx.grad, g.grad, b.grad]


def _case(N, C, dhw, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C, *dhw, generator=g) * 1.5 + 0.3).to(DEV).contiguous(memory_format=torch.channels_last_3d)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    dy = torch.randn(N, C, *dhw, generator=g).to(DEV).contiguous(memory_format=torch.channels_last_3d)
    return x, gamma, beta, dy


def _check_vs_fp64(outs, x, gamma, beta, dy, what):
    from oracle import fp64_ops as O
    y, dx, dg, db = [t.cpu().to(D64) for t in outs]
    y64, z64, xhat, rstd = O.instnorm_lrelu_fwd(x.cpu().to(D64), gamma.cpu().to(D64), beta.cpu().to(D64))
    mask = outs[0].cpu() > 0  # the LeakyReLU branches the HIP forward took
    flips = mask != (z64 > 0)
    if int(flips.sum()):
        assert float(z64[flips].abs().max()) <= 1e-5, f"{what}: LeakyReLU branch differs from fp64 away from zero"
    dx64, dg64, db64 = O.instnorm_lrelu_bwd(dy.cpu().to(D64), xhat, rstd, gamma.cpu().to(D64), mask)
    ey = float((y - y64).abs().max())
    edx, edg, edb = (float((a - r).abs().max()) / max(float(r.abs().max()), 1e-30)
                     for a, r in ((dx, dx64), (dg, dg64), (db, db64)))
    print(f"[{what}] y {ey:.1e} dx {edx:.1e} dgamma {edg:.1e} dbeta {edb:.1e}")
    assert ey <= 2e-6 * max(1.0, float(y64.abs().max())), f"{what}: y {ey:.2e}"
    assert edx <= 5e-6, f"{what}: dx {edx:.2e}"
    assert edg <= 1e-5 and edb <= 1e-5, f"{what}: dgamma {edg:.2e} dbeta {edb:.2e}"


# (N, C, spatial, single launches expected forward + backward at the default limit).  (2, 256, 16^3): 1 M elements per sample,
# over the limit (and 4096 voxels do not fit the registers); (3, 5, 3^3): C % 4 != 0 keeps the three-launch form; (1, 36, (5, 6, 7)): a last
# workgroup with one of four lanes in use, 210 voxels on 256 threads (rows past V); (2, 320, 4^3): one wave per workgroup;
# (2, 320, 8^3): the deepest stages of the benchmark network, four waves per workgroup
CASES = [(2, 320, (4, 4, 4), 2), (2, 256, (16, 16, 16), 0), (3, 5, (3, 3, 3), 0), (1, 36, (5, 6, 7), 2), (2, 320, (8, 8, 8), 2)]


@pytest.mark.parametrize("N,C,dhw,expect", CASES)
def test_instnorm_single_launch_vs_fp64(N, C, dhw, expect):
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import query
    x, gamma, beta, dy = _case(N, C, dhw, 11 + C)
    before = query("mvd_instnorm_single_launches")
    outs = _run(ops, x, gamma, beta, dy)
    assert query("mvd_instnorm_single_launches") - before == expect
    _check_vs_fp64(outs, x, gamma, beta, dy, f"N={N} C={C} {dhw}")
    for n, u, v in zip(("y", "dx", "dgamma", "dbeta"), outs, _run(ops, x, gamma, beta, dy)):
        assert torch.equal(u, v), f"{n}: run-to-run"


def test_instnorm_single_launch_limit_and_register_bounds():
    """V x C exactly at the limit takes the single launch, one voxel more does not; whatever the limit says, the kernels hold
    1024 voxels (256 threads x 16 rows / 4 lanes).  Both forms agree with fp64 on every shape, and with each other to the
    bars (their sums differ in association only)."""
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, query
    C = 32
    # the shipped default (profiles/r11_instnorm_small.txt): 327 680 elements per sample, at most 1024 voxels
    assert query("mvd_instnorm_single_launch", 1024, 320) == 1 and query("mvd_instnorm_single_launch", 1024, 324) == 0
    try:
        call("mvd_set_instnorm_small_max", 1000 * C)
        assert query("mvd_instnorm_single_launch", 1000, C) == 1 and query("mvd_instnorm_single_launch", 1001, C) == 0
        for dhw, expect in (((10, 10, 10), 2), ((7, 11, 13), 0)):  # 1000 voxels: at the limit; 1001: just above
            x, gamma, beta, dy = _case(2, C, dhw, 5)
            before = query("mvd_instnorm_single_launches")
            outs = _run(ops, x, gamma, beta, dy)
            assert query("mvd_instnorm_single_launches") - before == expect, dhw
            _check_vs_fp64(outs, x, gamma, beta, dy, f"limit {dhw}")
        # the backward workgroups walk the batch one sample after the other: past two samples the limit shrinks with 2 / N
        # (500 voxels: N = 4 counts 500 * 32 * 2 = 32 000 elements, at the limit; N = 5 counts 40 000: forward only)
        for N, expect in ((4, 2), (5, 1)):
            x, gamma, beta, dy = _case(N, C, (5, 10, 10), 7)
            before = query("mvd_instnorm_single_launches")
            outs = _run(ops, x, gamma, beta, dy)
            assert query("mvd_instnorm_single_launches") - before == expect, N
            _check_vs_fp64(outs, x, gamma, beta, dy, f"batch {N}")
        call("mvd_set_instnorm_small_max", 1 << 40)
        assert query("mvd_instnorm_single_launch", 1024, C) == 1 and query("mvd_instnorm_single_launch", 1025, C) == 0
        assert query("mvd_instnorm_single_launch", 64, 5) == 0
        # 1024 voxels: every thread holds its sixteen rows; 1025: three launches
        for dhw, expect in (((8, 8, 16), 2), ((5, 5, 41), 0)):
            x, gamma, beta, dy = _case(1, C, dhw, 6)
            before = query("mvd_instnorm_single_launches")
            outs = _run(ops, x, gamma, beta, dy)
            assert query("mvd_instnorm_single_launches") - before == expect, dhw
            _check_vs_fp64(outs, x, gamma, beta, dy, f"wide {dhw}")
            call("mvd_set_instnorm_small_max", 0)
            three = _run(ops, x, gamma, beta, dy)
            call("mvd_set_instnorm_small_max", 1 << 40)
            assert query("mvd_instnorm_single_launches") - before == expect
            assert float((outs[0] - three[0]).abs().max()) <= 2e-6 * max(1.0, float(three[0].abs().max()))
            assert float((outs[1] - three[1]).abs().max()) <= 5e-6 * float(three[1].abs().max())
    finally:
        call("mvd_set_instnorm_small_max", -1)
