"""GPU tests of the segmentation head (csrc/loss.hip: k_seghead_fwd, k_seghead_fwd_vox, k_seghead_fwd_voxp<2,4,8>,
k_seghead_dx, k_seghead_dx4, k_seghead_dw, k_seghead_dw4, k_seghead_dw4v, fp32 and bf16 input, the loader-prologue forms, and
the InstanceNorm backward kernels of csrc/instnorm.hip that consume the head's weight) at every class count K = 1..8 and at
the channel widths and volumes of tests/seghead_ref.py, where tests/test_seghead_cases_host.py checks on the CPU which kernel
each case runs.

Two comparisons, both through ops.SegHeadFn:
  * small integers (x, w in [-2, 2], b in [-3, 3], dl in [-1, 1]): every sum is exact in fp32 in any order and dx is exact
    in bf16, so logits, dx, dW and db must EQUAL the CPU result -- this is what catches an indexing error;
  * random data against oracle/fp64_ops.py on the same inputs (bf16-rounded x for the bf16 runs): fp32 outputs within
    1e-5 of the reference's largest magnitude per tensor; a bf16 dx gets one bf16 ulp, 2^-7 |ref|, on top:
    the fp32 sum and the fp64 sum may round to neighbouring bf16 values.
Every device evaluation runs twice and must repeat bit for bit.  The raw entry points are called only where an operand has to
be misaligned, where `accumulate` is set by hand, or where one output is not asked for."""
import ctypes

import pytest
import torch

import seghead_ref as S
from multimodal_mvd_seg_amd import ops
from multimodal_mvd_seg_amd._lib import call, query
from oracle import fp64_ops as O

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
CL3D = torch.channels_last_3d
D64, BF16 = torch.float64, torch.bfloat16
TOL = 1e-5            # of max|reference|, per tensor
BF16_ULP = 2.0 ** -7  # of |reference|, per element, bf16 outputs only
NAMES = ("logits", "dx", "dW", "db")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


# ------------------------------------------------------------------------------------------------ helpers
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_dev(x, dtype):
    """host NDHWC activation -> device, strides kept, bf16 for the bf16 runs"""
    t = x.to(DEV)
    t = t.to(BF16) if dtype == "bf16" else t
    assert ops._is_cl3d(t) and t.data_ptr() % 16 == 0
    return t


def twice(fn):
    a, b = fn(), fn()
    for n, u, v in zip(NAMES, a, b):
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), f"{n} differs between two runs"
    return a


def run_head(data, dtype, need_dx=True):
    """ops.SegHeadFn forward + backward, twice: (logits, dx or None, dW, db) on the host"""
    x, w, b, dl = data
    gx, gw, gb, gdl = to_dev(x, dtype), w.to(DEV), b.to(DEV), dl.to(DEV)

    def once():
        lx, lw, lb = gx.detach().requires_grad_(need_dx), gw.detach().requires_grad_(), gb.detach().requires_grad_()
        y = ops.SegHeadFn.apply(lx, lw, lb)
        y.backward(gdl)
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and lw.grad.dtype == torch.float32
        assert lx.grad is None or (lx.grad.dtype == gx.dtype and ops._is_cl3d(lx.grad))
        return y.detach().cpu(), (None if lx.grad is None else lx.grad.cpu()), lw.grad.cpu(), lb.grad.cpu()
    return twice(once)


def raw_fwd(x, w2, b, dtype, N, V, C, K, sp):
    logits = torch.empty((N, K, *sp), dtype=torch.float32, device=DEV)
    call("mvd_seghead_fwd_bf16" if dtype == "bf16" else "mvd_seghead_fwd", _p(x), _p(w2), _p(b), _p(logits), N, V, C, K, _stream())
    return logits


def raw_bwd(x, w2, dl, dx, dtype, N, V, C, K, accumulate=0, want_dw=True):
    dw = torch.empty((K, C), dtype=torch.float32, device=DEV) if want_dw else None
    db = torch.empty((K,), dtype=torch.float32, device=DEV) if want_dw else None
    ws = torch.empty(query("mvd_seghead_bwd_workspace_bytes", N, V, C, K), dtype=torch.uint8, device=DEV)
    call("mvd_seghead_bwd_bf16" if dtype == "bf16" else "mvd_seghead_bwd", _p(x), _p(w2), _p(dl), _p(dx), _p(dw), _p(db), N, V, C, K,
         accumulate, _p(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    return dw, db


def align_mask(x, w, dl, dx):
    return sum(bit for bit, t in zip((S.AL_X, S.AL_W, S.AL_DL, S.AL_DX), (x, w, dl, dx)) if t is None or t.data_ptr() % 16 == 0)


def paths(N, V, C, K, aligned=S.ALIGNED):
    return tuple(query(f"mvd_seghead_{d}_path", N, V, C, K, aligned) for d in ("fwd", "dx", "dw"))


def check_exact(got, want, what):
    for n, u, r in zip(NAMES, got, want):
        if u is None:
            continue
        assert u.shape == r.shape, (what, n, tuple(u.shape), tuple(r.shape))
        u = u.float()
        assert torch.equal(u, r), (f"{what}: {n}: {int((u != r).sum())} of {u.numel()} values differ, "
                                   f"max {float((u - r).abs().max())}")


def err_of(u, r):
    """(error as a fraction of its bar, error / max|ref|) of one tensor against its fp64 reference"""
    assert u.shape == r.shape and bool(torch.isfinite(u).all())
    m = float(r.abs().max())
    d = (u.to(D64) - r).abs()
    bar = TOL * m + (BF16_ULP * r.abs() if u.dtype == BF16 else 0.0)
    return float((d / bar).max()), float(d.max()) / max(m, 1e-300)


def check_close(got, want, what):
    errs = {n: err_of(u, r) for n, u, r in zip(NAMES, got, want) if u is not None}
    print(f"[{what}] " + " ".join(f"{n} {e[1]:.2e} ({e[0]:.3f} of bar)" for n, e in errs.items()))
    for n, (frac, _) in errs.items():
        assert frac <= 1.0, f"{what}: {n}: {frac:.3f} of the bar"


def tag(c, dtype):
    return f"{S.case_id(c)} {dtype} fwd{c.fwd} dx{c.dx} dw{c.dw}"


# ================================================================================================ 1. the case table
@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_integer_data_is_bit_exact(c, dtype):
    assert paths(c.N, S.vol(c), c.C, c.K) == (c.fwd, c.dx, c.dw)
    data, want = S.integer_case(c)
    check_exact(run_head(data, dtype), want, tag(c, dtype))


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_random_data_against_fp64(c, dtype):
    data, want = S.random_case(c, dtype)
    check_close(run_head(data, dtype), want, tag(c, dtype))


# ================================================================================================ 2. further cases
ACC = [S.Case(3, (4, 6, 10), 32, 5, None, 1, None),     # dx4, 8 rows
       S.Case(1, (4, 6, 10), 320, 3, None, 1, None),    # dx4, 3 rows of 80 groups, 16 idle threads
       S.Case(5, (2, 2, 2), 12, 8, None, 1, None),      # dx4, 85 rows, two quads per sample
       S.Case(3, (5, 7, 9), 32, 5, None, 0, None),      # generic: V % 4 != 0 (the low-resolution deep-supervision heads)
       S.Case(1, (5, 7, 9), 320, 8, None, 0, None),
       S.Case(2, (4, 6, 10), 33, 7, None, 0, None)]     # generic: C % 4 != 0


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("c", ACC, ids=S.case_id)
def test_accumulate_adds_to_what_dx_holds(c, dtype):
    """accumulate = 1 (the gradient-sharing join of ops.SegHeadFn) into both dx kernels: old + dx.  Integers: |old| <= 2 and
    |dx| <= 2 K, at most 18, exact in bf16.  Random: old + dx_ref in fp64, the same bars."""
    N, V, C, K = c.N, S.vol(c), c.C, c.K
    tdt = BF16 if dtype == "bf16" else torch.float32
    for kind in ("integer", "random"):
        (x, w, b, dl), (_, dx_ref, dw_ref, db_ref) = S.integer_case(c) if kind == "integer" else S.random_case(c, dtype)
        g = torch.Generator().manual_seed(K * 100 + C)
        old = S.ints(g, (N, *c.sp, C), -2, 2) if kind == "integer" else torch.randn((N, *c.sp, C), generator=g).to(tdt).float()
        old = old.permute(0, 4, 1, 2, 3)
        gx, gw, gdl = to_dev(x, dtype), w.to(DEV).view(K, C), dl.to(DEV)

        def once():
            dx = to_dev(old, dtype).clone(memory_format=torch.preserve_format)
            assert paths(N, V, C, K, align_mask(gx, gw, gdl, dx))[1] == c.dx
            dw, db = raw_bwd(gx, gw, gdl, dx, dtype, N, V, C, K, accumulate=1)
            return None, dx.cpu(), dw.cpu().view_as(dw_ref), db.cpu()
        got = twice(once)
        want = (None, old.to(dx_ref.dtype) + dx_ref, dw_ref, db_ref)
        if kind == "integer":
            check_exact(got, want, f"accumulate {S.case_id(c)} {dtype}")
        else:
            check_close(got, want, f"accumulate {S.case_id(c)} {dtype} dx{c.dx}")


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("c", [S.Case(3, (4, 6, 10), 96, 6, 2, 1, 2), S.Case(3, (5, 7, 9), 33, 4, 0, 0, 0)], ids=S.case_id)
def test_an_output_that_is_not_requested_is_not_needed(c, dtype):
    """x without a gradient (ops.SegHeadFn passes dx = NULL) and, through the raw entry point, dw = dbias = NULL"""
    N, V, C, K = c.N, S.vol(c), c.C, c.K
    data, want = S.integer_case(c)
    got = run_head(data, dtype, need_dx=False)
    assert got[1] is None
    check_exact(got, want, f"no dx {S.case_id(c)} {dtype}")
    x, w, b, dl = data
    gx, gw, gdl = to_dev(x, dtype), w.to(DEV).view(K, C), dl.to(DEV)

    def once():
        dx = torch.empty_like(gx)
        assert raw_bwd(gx, gw, gdl, dx, dtype, N, V, C, K, want_dw=False) == (None, None)
        return None, dx.cpu(), None, None
    check_exact(twice(once), want, f"no dW {S.case_id(c)} {dtype}")


def off_boundary(t):
    """the same values in the same layout one float (4 bytes) off a 16-byte boundary"""
    per = 4 // t.element_size()
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[per:per + t.numel()].as_strided(t.shape, t.stride())
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.stride() == t.stride()
    return v


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("c", [S.Case(3, (4, 6, 10), 32, 5, 0, 1, 0), S.Case(1, (4, 6, 10), 64, 8, 0, 1, 0),
                               S.Case(1, (5, 7, 9), 320, 2, 0, 0, 0)], ids=S.case_id)
def test_x_off_a_16_byte_boundary_takes_the_generic_forward_and_weight_gradient(c, dtype):
    N, V, C, K = c.N, S.vol(c), c.C, c.K
    assert paths(N, V, C, K)[0] != 0 and paths(N, V, C, K)[2] != 0       # aligned, the case would run the fast kernels
    for kind in ("integer", "random"):
        (x, w, b, dl), want = S.integer_case(c) if kind == "integer" else S.random_case(c, dtype)
        gx, gw, gb, gdl = off_boundary(to_dev(x, dtype)), w.to(DEV).view(K, C), b.to(DEV), dl.to(DEV)

        def once():
            dx = torch.empty(gx.shape, dtype=gx.dtype, device=DEV, memory_format=CL3D)
            assert paths(N, V, C, K, align_mask(gx, gw, gdl, dx)) == (c.fwd, c.dx, c.dw)
            y = raw_fwd(gx, gw, gb, dtype, N, V, C, K, c.sp)
            dw, db = raw_bwd(gx, gw, gdl, dx, dtype, N, V, C, K)
            return y.cpu(), dx.cpu(), dw.cpu().view_as(want[2]), db.cpu()
        got = twice(once)
        (check_exact if kind == "integer" else check_close)(got, want, f"misaligned x {S.case_id(c)} {dtype} fwd0 dx{c.dx} dw0")


def test_more_classes_than_the_kernels_hold_and_none_are_refused():
    N, V, C = 1, 64, 32
    x = torch.zeros(N, V, C, device=DEV)
    w, b = torch.zeros(9, C, device=DEV), torch.zeros(9, device=DEV)
    lg = torch.zeros(N, 9, V, device=DEV)
    dx, dw, db = torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(b)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for K in (9, 0):
        for bf in ("", "_bf16"):
            with pytest.raises(RuntimeError, match=r"seghead_fwd: bad shape \(K<=8\)"):
                call("mvd_seghead_fwd" + bf, _p(x), _p(w), _p(b), _p(lg), N, V, C, K, None)
            with pytest.raises(RuntimeError, match=r"seghead_bwd: bad shape \(K<=8\)"):
                call("mvd_seghead_bwd" + bf, _p(x), _p(w), _p(lg), _p(dx), _p(dw), _p(db), N, V, C, K, 0, _p(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in (lg, dx, dw, db))


def test_generic_dx_refuses_a_weight_tile_beyond_the_lds():
    """k_seghead_dx stages w [K][C] and 64 voxels of dl in (K C + 64 K) floats of dynamic LDS: 67 712 bytes at K = 8, C = 2052.
    The host check refuses it with the project's own message; no kernel runs."""
    N, V, K = 1, 4, 8
    for C in (2052, 2048):
        assert paths(N, V, C, K)[1] == 0 and (K * C + 64 * K) * 4 > 64 * 1024
        x, w = torch.zeros(N, V, C, device=DEV), torch.zeros(K, C, device=DEV)
        dl, dx = torch.zeros(N, K, V, device=DEV), torch.full((N, V, C), 7.0, device=DEV)
        ws = torch.empty(query("mvd_seghead_bwd_workspace_bytes", N, V, C, K), dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match="seghead_bwd: K x C too large for the LDS weight tile"):
            call("mvd_seghead_bwd", _p(x), _p(w), _p(dl), _p(dx), None, None, N, V, C, K, 0, _p(ws), ws.numel(), None)
        torch.cuda.synchronize()
        assert bool((dx == 7.0).all())
    assert (7 * 2052 + 64 * 7) * 4 <= 64 * 1024   # (one class fewer fits)


# ================================================================================================ 3. two large cases
def test_forward_per_voxel_kernel_at_two_to_the_twenty_voxels():
    """C = 64 at N V = 2^20: k_seghead_fwd_vox with two whole 32-channel chunks (below that size C = 64 runs voxp<2>)"""
    c = S.BIG_FWD
    N, V, C, K = c.N, S.vol(c), c.C, c.K
    assert N * V == 1 << 20 and paths(N, V, C, K)[0] == 1 and paths(N, V - 1, C, K)[0] == 2
    g = torch.Generator().manual_seed(64)
    x = torch.randint(-2, 3, (N, *c.sp, C), generator=g, dtype=torch.int8)
    w, b = S.ints(g, (K, C), -2, 2), S.ints(g, (K,), -3, 3)
    want = (x.view(V, C).float() @ w.t() + b).t().reshape(N, K, *c.sp)     # |sum| <= 4 * 64 + 3: exact in fp32
    gw, gb = w.to(DEV).view(K, C, 1, 1, 1), b.to(DEV)
    for dtype in S.DTYPES:
        gx = to_dev(x.to(DEV).float().permute(0, 4, 1, 2, 3), dtype)
        with torch.no_grad():
            y = [ops.SegHeadFn.apply(gx, gw, gb).cpu() for _ in range(2)]
        assert torch.equal(y[0], y[1]), "run-to-run"
        assert torch.equal(y[0], want), f"{dtype}: {int((y[0] != want).sum())} logits differ"


def test_dx4_grid_stride_loop_takes_a_second_trip():
    """C = 32, V = 66 x 128 x 128: 270 336 quads over 32 rows per block want 8448 blocks, 8192 are launched, so the first 256
    blocks go round the loop twice.  dx only (raw entry point, dw = NULL; x is not read)."""
    c = S.BIG_DX
    N, V, C, K = c.N, S.vol(c), c.C, c.K
    assert V // 4 == 270336 and -(-(V // 4) // (256 // (C // 4))) == 8448 and paths(N, V, C, K)[1] == 1
    g = torch.Generator().manual_seed(66)
    dl, w = S.ints(g, (N, K, V), -1, 1), S.ints(g, (K, C), -2, 2)
    want = dl[0].t() @ w                                                   # [V, C], |sum| <= 4
    gdl, gw = dl.to(DEV), w.to(DEV)
    for dtype in S.DTYPES:
        x = torch.empty((N, V, C), dtype=BF16 if dtype == "bf16" else torch.float32, device=DEV)

        def once():
            dx = torch.empty_like(x)
            raw_bwd(x, gw, gdl, dx, dtype, N, V, C, K, want_dw=False)
            return dx
        a, b = once(), once()
        assert torch.equal(a, b), "run-to-run"
        a = a.cpu().float().view(V, C)
        assert torch.equal(a, want), f"{dtype}: {int((a != want).sum())} values differ"


# ================================================================================================ 4. the fused forms at every K
FUSED_C = (32, 64, 96, 320)
# the volumes of tests/test_gpu_norm_bwd_from_dl.py (8x8x12 x 2, 4x6x10, 12x16x20: 7 statistics blocks, 15 apply blocks) and of
# tests/test_gpu_fused_block.py (33x36x44, 64^3 x 2), and 5 samples of 2x2x2: every K at every width on each
FUSED_VOLUMES = ((1, (4, 6, 10)), (5, (2, 2, 2)), (2, (8, 8, 12)), (1, (12, 16, 20)), (1, (33, 36, 44)), (2, (64, 64, 64)))
BIG = (64, 64, 64)   # device only: no CPU reference (tests/test_gpu_norm_bwd_from_dl.py does not take it against fp64 either)
FUSED = [(N, sp, C, K) for N, sp in FUSED_VOLUMES for C in FUSED_C for K in range(1, 9)]
FUSED_FP64 = [f for f in FUSED if f[1] != BIG]
FNAMES = ["logits", "dy0", "dgamma", "dbeta", "dW", "db"]


def _fused_id(f):
    return f"N{f[0]}-{'x'.join(map(str, f[1]))}-C{f[2]}-K{f[3]}"


def _fused_inputs(N, sp, C, K, dtype):
    seed = N * 1000 + sp[0] * 100 + sp[2] + C * 7 + K
    # (64^3 is compared on the device only: drawn there, up to 168 M values per case)
    g = (torch.Generator(device=DEV) if sp == BIG else torch.Generator()).manual_seed(seed)
    y0 = (torch.randn(N, *sp, C, generator=g, device=g.device) * 1.5 + 0.3).to(BF16 if dtype == "bf16" else torch.float32)
    y0 = y0.to(DEV).permute(0, 4, 1, 2, 3)
    gamma = (torch.rand(C, generator=g, device=g.device) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g, device=g.device) * 0.2).to(DEV)
    w = (torch.randn(K, C, 1, 1, 1, generator=g, device=g.device) * 0.2).to(DEV)
    b = (torch.randn(K, generator=g, device=g.device) * 0.1).to(DEV)
    gl = torch.randn(N, K, *sp, generator=g, device=g.device).to(DEV)
    assert ops._is_cl3d(y0)
    return y0, gamma, beta, w, b, gl


def _three_launch_instnorm(fn, switch=True):
    """The fused forms mirror the THREE-launch InstanceNorm kernels.  Where the un-fused node would take the single-launch
    kernels instead (mvd_instnorm_single_launch: V C <= 327 680 per sample; another grid, another order of the fp64 sums, so
    other last bits of mean / rstd), that path is switched off, as tests/test_gpu_norm_bwd_from_dl.py does.  switch = False:
    the default setting."""
    if not switch:
        return fn()
    call("mvd_set_instnorm_small_max", 0)
    try:
        return fn()
    finally:
        call("mvd_set_instnorm_small_max", -1)


def _run_fused(inputs, fused, bf, from_dl=None, calls=None, switch=True):
    y0, gamma, beta, w, b, gl = inputs
    saved, orig_call = ops.NORM_BWD_FROM_DL[0], ops.call

    def counting_call(name, *a, **k):
        calls[name] = calls.get(name, 0) + 1
        return orig_call(name, *a, **k)

    def go():
        ps = [t.clone().requires_grad_() for t in (gamma, beta, w, b)]
        yy = y0.clone(memory_format=torch.preserve_format).requires_grad_()
        if fused:
            lg = ops.NormActSegHeadFn.apply(yy, ps[0], ps[1], 1e-5, 0.01, ps[2], ps[3])
        else:
            lg = ops.SegHeadFn.apply(ops.InstanceNormLeakyReLUFn.apply(yy, ps[0], ps[1], 1e-5, 0.01, bf), ps[2], ps[3])
        lg.backward(gl)
        torch.cuda.synchronize()
        return [lg.detach(), yy.grad] + [p.grad for p in ps]
    if from_dl is not None:
        ops.NORM_BWD_FROM_DL[0] = from_dl
    if calls is not None:
        ops.call = counting_call
    try:
        return _three_launch_instnorm(go, switch)
    finally:
        ops.NORM_BWD_FROM_DL[0] = saved
        ops.call = orig_call


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("f", FUSED, ids=_fused_id)
def test_norm_act_seghead_node_is_bit_identical_to_the_two_separate_nodes_at_every_k(f, dtype):
    """ops.NormActSegHeadFn against InstanceNormLeakyReLUFn -> SegHeadFn on the same raw conv output, as
    tests/test_gpu_fused_block.py does at C = 32, K = 5: logits, d y0, d gamma, d beta, dW, db bit for bit.  Under the default
    setting wherever the chain runs the three-launch InstanceNorm by itself (V C > 327 680 per sample: 33x36x44 and 64^3 at
    every width, 12x16x20 from 96 channels on); below that the chain's single-launch
    statistics differ from the node's in the last bits by construction and that path is switched off for the comparison."""
    N, sp, C, K = f
    inputs = _fused_inputs(N, sp, C, K, dtype)
    assert ops.fused_norm_seghead_ok(inputs[0], inputs[3])
    small = query("mvd_instnorm_single_launch", sp[0] * sp[1] * sp[2], C) == 1
    assert not small or sp[0] * sp[1] * sp[2] * C <= 327680     # (the default limit; the large volumes run as production does)
    fused = _run_fused(inputs, True, dtype == "bf16", switch=small)
    chain = _run_fused(inputs, False, dtype == "bf16", switch=small)
    for n, u, v in zip(FNAMES, fused, chain):
        assert u.dtype == v.dtype and torch.equal(u, v), f"{n}: {int((u != v).sum())} of {u.numel()} values differ"


@pytest.mark.parametrize("f", FUSED_FP64, ids=_fused_id)
def test_norm_bwd_from_logit_gradient_equals_the_stored_form_and_fp64_at_every_k(f):
    """mvd_instnorm_lrelu_bwd_head (k_in_bwd_stats<4,false,false,HK>, k_in_bwd_apply_rows<false,false,HK>, HK = K) against the
    two-call form bit for bit and against fp64 within relative L2 1e-5, as tests/test_gpu_norm_bwd_from_dl.py does at K = 5"""
    N, sp, C, K = f
    inputs = _fused_inputs(N, sp, C, K, "fp32")
    y0, gamma, beta, w, b, gl = inputs
    assert ops.fused_norm_seghead_ok(y0, w)
    on_calls, off_calls = {}, {}
    on = _run_fused(inputs, True, False, True, on_calls)
    off = _run_fused(inputs, True, False, False, off_calls)
    assert on_calls.get("mvd_instnorm_lrelu_bwd_head") == 1 and "mvd_instnorm_lrelu_bwd" not in on_calls, on_calls
    assert off_calls.get("mvd_instnorm_lrelu_bwd") == 1 and "mvd_instnorm_lrelu_bwd_head" not in off_calls, off_calls
    for n, u, v in zip(FNAMES, on, off):
        assert torch.equal(u, v), f"{n}: {int((u != v).sum())} of {u.numel()} values differ between the two forms"
    for n, u, v in zip(FNAMES, on, _run_fused(inputs, True, False, True)):
        assert torch.equal(u, v), f"{n}: run-to-run"
    # fp64 oracle, LeakyReLU branches as the HIP forward took them (bit-identical un-fused apply pass)
    y_h = _three_launch_instnorm(lambda: ops.InstanceNormLeakyReLUFn.apply(y0, gamma, beta, 1e-5, 0.01)).cpu()
    x64, gl64 = y0.cpu().to(D64), gl.cpu().to(D64)
    a64, z64, xhat, rstd = O.instnorm_lrelu_fwd(x64, gamma.cpu().to(D64), beta.cpu().to(D64))
    mask = y_h > 0
    flips = mask != (z64 > 0)
    if int(flips.sum()):
        assert float(z64[flips].abs().max()) <= 1e-5, "LeakyReLU branch differs from fp64 away from zero"
        a64 = torch.where(mask, z64, z64 * 0.01)
    lg64 = O.seghead_fwd(a64, w.cpu(), b.cpu())
    da64, dw64, db64 = O.seghead_bwd(a64, w.cpu(), gl64)
    dx64, dg64, dbe64 = O.instnorm_lrelu_bwd(da64, xhat, rstd, gamma.cpu().to(D64), mask)
    errs = {}
    for n, u, r in zip(FNAMES, on, [lg64, dx64, dg64, dbe64, dw64, db64]):
        u = u.detach().cpu().to(D64)
        assert u.shape == r.shape, (n, tuple(u.shape), tuple(r.shape))
        errs[n] = float((u - r).norm() / (r.norm() + 1e-300))
    print(f"[fused {_fused_id(f)}] " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 1e-5, f"{k}: relative L2 error {v:.2e} vs fp64"


# ================================================================================================ 5. layout transposes
@pytest.mark.parametrize("C", [1, 3, 4, 5, 33, 70])
def test_layout_transposes_equal_permute(C):
    """k_nchw_to_ndhwc (and its C == 4 form) and k_ndhwc_to_nchw, the first and last step of ops.SegHeadFn for planar operands,
    against permute().contiguous(), bit for bit"""
    N = 3
    for V, sp in ((1, (1, 1, 1)), (31, (1, 1, 31)), (33, (1, 3, 11)), (315, (5, 7, 9))):
        g = torch.Generator().manual_seed(C * 1000 + V)
        planar = torch.randn(N, C, V, generator=g).to(DEV)
        rows = torch.full((N, V, C), float("nan"), device=DEV)
        call("mvd_nchw_to_ndhwc", _p(planar), _p(rows), N, C, V, _stream())
        assert torch.equal(rows, planar.permute(0, 2, 1).contiguous()), (C, V, "to NDHWC")
        back = torch.full((N, C, V), float("nan"), device=DEV)
        call("mvd_ndhwc_to_nchw", _p(rows), _p(back), N, C, V, _stream())
        assert torch.equal(back, planar), (C, V, "to planar")
        if C == 4:   # a destination off the 16-byte boundary takes the tiled kernel instead of the float4 one
            buf = torch.full((N * V * C + 8,), float("nan"), device=DEV)
            call("mvd_nchw_to_ndhwc", _p(planar), _p(buf[1:]), N, C, V, _stream())
            assert torch.equal(buf[1:1 + N * V * C].view(N, V, C), rows) and bool(buf[0].isnan()) and bool(buf[1 + N * V * C:].isnan().all())
        if C > 1 and V > 1:   # (one channel or one voxel is both layouts at once: the ops return the tensor itself)
            t5 = planar.view(N, C, *sp)
            cl = ops.to_ndhwc(t5)
            assert ops._is_cl3d(cl) and cl.data_ptr() != t5.data_ptr() and torch.equal(cl, t5)
            assert torch.equal(cl.permute(0, 2, 3, 4, 1).contiguous().view(N, V, C), rows)
            pl = ops.to_planar(cl)
            assert pl.is_contiguous() and pl.data_ptr() != cl.data_ptr() and torch.equal(pl.view(N, C, V), planar)
