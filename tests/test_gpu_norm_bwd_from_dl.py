"""The fp32 backward of ops.NormActSegHeadFn without the stored d a: mvd_instnorm_lrelu_bwd_head forms
d a[v][c] = sum_k dl[k][v] * w[k][c] inside the two InstanceNorm backward passes (the expression and k order of the head's
input-gradient kernel, the grids and chunks of mvd_instnorm_lrelu_bwd), so every gradient must equal the two-call form
(ops.NORM_BWD_FROM_DL off) bit for bit, and both must sit within the fp64 bars of the un-fused blocks
(tests/test_gpu_cfg2.py: InstanceNorm block and seg head block, relative L2 <= 1e-5).  The head form mirrors the THREE-launch
kernels; the small shapes here would take the single-launch backward with the switch off (other grid, other order of the
fp64 sums), so that path is switched off for the comparison (mvd_set_instnorm_small_max(0))."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
D64 = torch.float64
CL = torch.channels_last_3d
NAMES = ["logits", "dy0", "dgamma", "dbeta", "dW", "db"]


def rel_l2(a, ref):
    a, ref = a.detach().cpu().to(D64), ref.detach().cpu().to(D64)
    assert a.shape == ref.shape, (tuple(a.shape), tuple(ref.shape))
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def _inputs(N, dhw, C=32, K=5):
    g = torch.Generator().manual_seed(N * 1000 + dhw[0] * 100 + dhw[2])
    y0 = (torch.randn(N, C, *dhw, generator=g) * 1.5 + 0.3).to(DEV).contiguous(memory_format=CL)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    w = (torch.randn(K, C, 1, 1, 1, generator=g) * 0.2).to(DEV)
    b = (torch.randn(K, generator=g) * 0.1).to(DEV)
    gl = torch.randn(N, K, *dhw, generator=g).to(DEV)
    return y0, gamma, beta, w, b, gl


def _run(ops, inputs, from_dl, calls=None):
    y0, gamma, beta, w, b, gl = inputs
    saved, orig_call = ops.NORM_BWD_FROM_DL[0], ops.call

    def counting_call(name, *a, **k):
        calls[name] = calls.get(name, 0) + 1
        return orig_call(name, *a, **k)
    ops.NORM_BWD_FROM_DL[0] = from_dl
    if calls is not None:
        ops.call = counting_call
    orig_call("mvd_set_instnorm_small_max", 0)  # the same-grid three-launch kernels on both sides
    try:
        ps = [t.clone().requires_grad_() for t in (gamma, beta, w, b)]
        yy = y0.clone().requires_grad_()
        lg = ops.NormActSegHeadFn.apply(yy, ps[0], ps[1], 1e-5, 0.01, ps[2], ps[3])
        lg.backward(gl)
        torch.cuda.synchronize()
    finally:
        orig_call("mvd_set_instnorm_small_max", -1)
        ops.NORM_BWD_FROM_DL[0] = saved
        ops.call = orig_call
    return [lg.detach(), yy.grad] + [p.grad for p in ps]


# two shapes with one block per sample (whole and ragged rows per thread) and one with several blocks per sample and a
# short last chunk (V = 3840: 7 statistics blocks of 549 voxels, 15 apply blocks)
@pytest.mark.parametrize("N,dhw", [(2, (8, 8, 12)), (1, (4, 6, 10)), (1, (12, 16, 20))])
def test_norm_bwd_from_logit_gradient_equals_the_stored_form_and_fp64(N, dhw):
    from multimodal_mvd_seg_amd import ops
    from oracle import fp64_ops as O
    inputs = _inputs(N, dhw)
    y0, gamma, beta, w, b, gl = inputs
    assert ops.fused_norm_seghead_ok(y0, w)
    on_calls, off_calls = {}, {}
    on = _run(ops, inputs, True, on_calls)
    off = _run(ops, inputs, False, off_calls)
    # which path ran
    assert on_calls.get("mvd_instnorm_lrelu_bwd_head") == 1 and "mvd_instnorm_lrelu_bwd" not in on_calls, on_calls
    assert off_calls.get("mvd_instnorm_lrelu_bwd") == 1 and "mvd_instnorm_lrelu_bwd_head" not in off_calls, off_calls
    for n, u, v in zip(NAMES, on, off):
        assert torch.equal(u, v), f"{n}: {int((u != v).sum())} of {u.numel()} values differ between the two forms"
    for n, u, v in zip(NAMES, on, _run(ops, inputs, True)):
        assert torch.equal(u, v), f"{n}: run-to-run"
    # fp64 oracle, LeakyReLU branches as the HIP forward took them (bit-identical un-fused apply pass)
    y_h = ops.InstanceNormLeakyReLUFn.apply(y0, gamma, beta, 1e-5, 0.01).cpu()
    x64, w64, gl64 = y0.cpu().to(D64), w.cpu().to(D64).view(5, -1), gl.cpu().to(D64)
    a64, z64, xhat, rstd = O.instnorm_lrelu_fwd(x64, gamma.cpu().to(D64), beta.cpu().to(D64))
    mask = y_h > 0
    flips = mask != (z64 > 0)
    if int(flips.sum()):
        assert float(z64[flips].abs().max()) <= 1e-5, "LeakyReLU branch differs from fp64 away from zero"
        a64 = torch.where(mask, z64, z64 * 0.01)
    lg64 = torch.einsum('kc,ncdhw->nkdhw', w64, a64) + b.cpu().to(D64).view(1, 5, 1, 1, 1)
    da64 = torch.einsum('kc,nkdhw->ncdhw', w64, gl64)
    dx64, dg64, dbe64 = O.instnorm_lrelu_bwd(da64, xhat, rstd, gamma.cpu().to(D64), mask)
    dw64 = torch.einsum('nkdhw,ncdhw->kc', gl64, a64).view(5, -1, 1, 1, 1)
    db64 = gl64.sum((0, 2, 3, 4))
    errs = {n: rel_l2(u, r) for n, u, r in zip(NAMES, on, [lg64, dx64, dg64, dbe64, dw64, db64])}
    print(f"[N={N} {dhw}] " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 1e-5, f"{k}: relative L2 error {v:.2e} vs fp64"


def test_logit_gradient_form_refuses_what_it_does_not_serve():
    """Host checks of the entry point: more classes than the kernels are built for, a missing head weight."""
    from multimodal_mvd_seg_amd import ops
    from multimodal_mvd_seg_amd._lib import call, query
    N, C, V = 1, 32, 64
    x = torch.randn(N, V, C, device=DEV)
    dl = torch.randn(N, 9, V, device=DEV)
    w = torch.randn(9, C, device=DEV)
    v = [torch.ones(C, device=DEV) for _ in range(2)] + [torch.zeros(N, C, device=DEV), torch.ones(N, C, device=DEV)]
    out = [torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)]
    ws = torch.empty(query("mvd_instnorm_workspace_bytes", N, V, C), dtype=torch.uint8, device=DEV)
    p = ops._p
    for wt, K in ((w, 9), (None, 5)):
        with pytest.raises(RuntimeError, match="instnorm_bwd"):
            call("mvd_instnorm_lrelu_bwd_head", p(x), p(dl), p(wt), K, *[p(t) for t in v], *[p(t) for t in out], N, V, C, 0.01,
                 p(ws), ws.numel(), None)
