"""Every InstanceNorm + LeakyReLU kernel path of csrc/instnorm.hip against oracle/fp64_ops.py at its geometry edges: the
case table of tests/instnorm_ref.py (tests/test_instnorm_cases_host.py checks on the CPU which kernels and edges each case
reaches), called through the C ABI so that the test owns every buffer.

  * workspace: 0xFF bytes before every call -- a block partial that a kernel did not write reads as NaN;
  * outputs: filled with a NaN sentinel and allocated with a guard tail: the tail must still hold the sentinel after the call,
    no element inside may;
  * mean, rstd: at most ONE float step from the fp64 value rounded to float (inputs with |mean| <= 2 std: fp64 sums of float
    data are far more exact than 2^-24, only the final rounding can differ) -- this is what a loss of fp64 accumulation fails;
  * fp32 y, dx, dgamma, dbeta: the bars of tests/test_gpu_instnorm_small.py (y 2e-6 max(1, max|y64|), dx 5e-6 max|dx64|,
    dgamma / dbeta 1e-5 of their maxima);
  * bf16 y: |y - y64| <= 2^-8 |y64| + 2e-6 max(1, max|y64|) per element, x64 the bf16-rounded input (round-to-nearest-even costs
    2^-9 relative; the factor two covers a rounding flipped by the fp32 error underneath); bf16 dx: the same form on the dx bar;
  * LeakyReLU branches: those of the HIP forward; they may differ from sign(z64) only where |z64| <= 1e-5.  The backward kernels
    re-compute z = fma((x - mean) rstd, gamma, beta) from the float mean / rstd; its sign is reproduced on the host exactly (the
    product of two floats is exact in fp64) and must equal the forward's branch wherever the forward used that expression (every
    path but bf16 -> bf16, whose forward is the scale / shift form and may differ from it where |z64| <= 1e-5);
  * every evaluation runs twice and must repeat bit for bit; the two launch counters move as the case's path says.
Nothing here may fault: every case is inside the entry points' documented domain, and the refusals are host checks that
launch nothing (the buffers they were handed are unchanged afterwards)."""
import ctypes

import pytest
import torch

import instnorm_ref as R
from multimodal_mvd_seg_amd import _lib, ops
from multimodal_mvd_seg_amd._lib import call, query

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
D64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32
GUARD = 1024                 # elements behind every output
NAN32, NAN16 = 0x7FC0DEAD, 0x7FDE   # quiet NaNs (as int32 / int16 bit patterns) no kernel produces


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    yield
    call("mvd_set_instnorm_small_max", -1)


# ------------------------------------------------------------------------------------------------ buffers the test owns
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Out:
    """an output of `shape` with a guard tail, everything filled with a NaN sentinel"""

    def __init__(self, shape, bf16=False):
        n = 1
        for s in shape:
            n *= s
        self.n, self.shape, self.bf16 = n, tuple(shape), bf16
        self.raw = torch.full((n + GUARD,), NAN16 if bf16 else NAN32, dtype=torch.int16 if bf16 else torch.int32, device=DEV)
        assert self.raw.data_ptr() % 16 == 0

    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr())

    def take(self, what):
        """the written tensor on the host (fp32 or bf16), after the sentinel checks"""
        raw = self.raw.cpu()
        s = NAN16 if self.bf16 else NAN32
        assert bool((raw[self.n:] == s).all()), f"{what}: written past its end"
        left = int((raw[:self.n] == s).sum())
        assert left == 0, f"{what}: {left} of {self.n} elements were not written"
        return raw[:self.n].view(BF16 if self.bf16 else F32).reshape(self.shape)


def workspace(N, V, C):
    return torch.full((query("mvd_instnorm_workspace_bytes", N, V, C),), 0xFF, dtype=torch.uint8, device=DEV)


def up(t, bf16=False):
    t = t.contiguous().to(DEV)
    t = t.to(BF16) if bf16 else t
    assert t.data_ptr() % 16 == 0
    return t


class Counters:
    def __init__(self):
        self.v = self.now()

    @staticmethod
    def now():
        return query("mvd_instnorm_single_launches"), query("mvd_instnorm_stats_pass_launches")

    def moved(self):
        a, self.v = self.v, self.now()
        return self.v[0] - a[0], self.v[1] - a[1]


# ------------------------------------------------------------------------------------------------ one evaluation of a case
def forward(c, g):
    """the forward of the case through its entry point(s): {y, mean, rstd} on the host (y None: statistics only)"""
    N, V, C = c.N, c.V, c.C
    xb, yb = c.xt == "bf16", c.yt == "bf16"
    mean, rstd = Out((N, C)), Out((N, C))
    y = None if (c.entry == "tiles" and not xb) else Out((N, V, C), yb)
    ws = workspace(N, V, C)
    cnt = Counters()
    if c.entry == "prestats":
        call("mvd_instnorm_lrelu_fwd_prestats", _p(g["x"]), _p(g["tiles"]), c.ntiles, _p(g["gamma"]), _p(g["beta"]), y.ptr(),
             mean.ptr(), rstd.ptr(), N, V, C, R.EPS, R.SLOPE, _p(ws), ws.numel(), _stream())
        want = (0, 0)
    elif c.entry == "tiles" and not xb:
        call("mvd_instnorm_stats_from_tiles", _p(g["tiles"]), c.ntiles, mean.ptr(), rstd.ptr(), N, V, C, R.EPS, _p(ws), ws.numel(),
             _stream())
        want = (0, 0)
    elif c.entry == "tiles":
        scale, shift = Out((N, C)), Out((N, C))
        call("mvd_instnorm_finalize_tiles", _p(g["tiles"]), c.ntiles, _p(g["gamma"]), _p(g["beta"]), mean.ptr(), rstd.ptr(),
             scale.ptr(), shift.ptr(), N, V, C, R.EPS, _stream())
        call("mvd_instnorm_lrelu_apply_bf16", _p(g["x"]), scale.ptr(), shift.ptr(), y.ptr(), N, V, C, R.SLOPE, _stream())
        want = (0, 0)
    elif not xb and not yb:
        call("mvd_instnorm_lrelu_fwd", _p(g["x"]), _p(g["gamma"]), _p(g["beta"]), y.ptr(), mean.ptr(), rstd.ptr(), N, V, C, R.EPS,
             R.SLOPE, _p(ws), ws.numel(), _stream())
        want = (1, 0) if c.fwd[0] == R.SMALL_FWD else (0, 1)
    else:
        call("mvd_instnorm_lrelu_fwd_bf16", _p(g["x"]), int(xb), _p(g["gamma"]), _p(g["beta"]), y.ptr(), mean.ptr(), rstd.ptr(), N,
             V, C, R.EPS, R.SLOPE, _p(ws), ws.numel(), _stream())
        want = (0, 1)
    torch.cuda.synchronize()
    assert cnt.moved() == want, f"{R.case_id(c)}: (single launches, statistics passes) moved by other than {want}"
    out = {"mean": mean.take("mean"), "rstd": rstd.take("rstd"), "y": y.take("y") if y else None}
    if c.entry == "tiles" and xb:
        out["scale"], out["shift"] = scale.take("scale"), shift.take("shift")
    return out


def backward(c, g, mean, rstd):
    N, V, C = c.N, c.V, c.C
    xb, yb = c.xt == "bf16", c.yt == "bf16"
    dx, dg, db = Out((N, V, C), xb), Out((C,)), Out((C,))
    ws = workspace(N, V, C)
    cnt = Counters()
    tail = (_p(g["gamma"]), _p(g["beta"]), _p(mean), _p(rstd), dx.ptr(), dg.ptr(), db.ptr(), N, V, C, R.SLOPE, _p(ws), ws.numel(),
            _stream())
    if c.entry == "head":
        call("mvd_instnorm_lrelu_bwd_head", _p(g["x"]), _p(g["dl"]), _p(g["hw"]), R.HEAD_K, *tail)
    elif not xb and not yb:
        call("mvd_instnorm_lrelu_bwd", _p(g["x"]), _p(g["dy"]), *tail)
    else:
        call("mvd_instnorm_lrelu_bwd_bf16", _p(g["x"]), int(xb), _p(g["dy"]), *tail)
    torch.cuda.synchronize()
    want = (1, 0) if c.bwd[0] == R.SMALL_BWD else (0, 0)
    assert cnt.moved() == want, f"{R.case_id(c)}: (single launches, statistics passes) moved by other than {want}"
    return {"dx": dx.take("dx"), "dgamma": dg.take("dgamma"), "dbeta": db.take("dbeta")}


def twice(fn, what):
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), \
            f"{what}: {k} differs between two runs"
    return a


def upload(c, d):
    xb, yb = c.xt == "bf16", c.yt == "bf16"
    g = {"x": up(d.x, xb), "gamma": up(d.gamma), "beta": up(d.beta)}
    if d.dy is not None:
        g["dy"] = up(d.dy, yb)
    if d.tiles is not None:
        g["tiles"] = up(d.tiles)
    if d.hw is not None:
        g["hw"], g["dl"] = up(d.hw), up(d.dl)
    return g


# ------------------------------------------------------------------------------------------------ the comparisons
def check_stats(c, d, f, what, steps=1):
    for k, ref in (("mean", d.mean), ("rstd", d.rstd)):
        u = R.ulps(f[k], ref.float())
        print(f"[{what}] {k}: {int(u.max())} float steps from fp64 at worst")
        assert int(u.max()) <= steps, f"{what}: {k} is {int(u.max())} float steps from the fp64 value"


def check_y(c, d, f, what):
    y = f["y"]
    y64, ymax = d.y, max(1.0, float(d.y.abs().max()))
    flips = (y.float() > 0) != (d.z > 0)
    if int(flips.sum()):
        assert float(d.z[flips].abs().max()) <= 1e-5, f"{what}: LeakyReLU branch differs from fp64 away from zero"
    e = (y.to(D64) - y64).abs()
    e = torch.where(flips, torch.zeros_like(e), e)     # (|z64| <= 1e-5: either branch is within the bar by construction)
    if y.dtype == BF16:
        bar = 2.0 ** -8 * y64.abs() + 2e-6 * ymax
        frac = float((e / bar).max())
        print(f"[{what}] bf16 y: {frac:.3f} of its bar at worst")
        assert frac <= 1.0, f"{what}: bf16 y at {frac:.3f} of |y64| / 256 + 2e-6 max(1, max|y64|)"
    else:
        print(f"[{what}] y: {float(e.max()) / ymax:.2e} of max(1, max|y64|)   (bar 2e-6)")
        assert float(e.max()) <= 2e-6 * ymax, f"{what}: y {float(e.max()):.2e}"


def bwd_mask(c, d, f, what):
    """the branches the backward kernels take: sign of fma((x - mean) rstd, gamma, beta) on the float mean / rstd, exact on the
    host; equal to the forward's where the forward computes the same expression"""
    xh = (d.x - f["mean"].unsqueeze(1)) * f["rstd"].unsqueeze(1)
    mask = (xh.to(D64) * d.gamma.to(D64) + d.beta.to(D64)) > 0
    if f["y"] is not None:
        differ = mask != (f["y"].float() > 0)
        if c.xt == "bf16":
            assert not int(differ.sum()) or float(d.z[differ].abs().max()) <= 1e-5, f"{what}: branches of the two forms"
        else:
            assert not int(differ.sum()), f"{what}: the backward would take {int(differ.sum())} branches the forward did not"
    flips = mask != (d.z > 0)
    assert not int(flips.sum()) or float(d.z[flips].abs().max()) <= 1e-5, f"{what}: LeakyReLU branch differs away from zero"
    return mask


def check_bwd(c, d, b, mask, what):
    dx64, dg64, db64 = R.bwd64(d, mask)
    dx = b["dx"]
    m = float(dx64.abs().max())
    e = (dx.to(D64) - dx64).abs()
    if dx.dtype == BF16:
        frac = float((e / (2.0 ** -8 * dx64.abs() + 5e-6 * m)).max())
        print(f"[{what}] bf16 dx: {frac:.3f} of its bar at worst")
        assert frac <= 1.0, f"{what}: bf16 dx at {frac:.3f} of |dx64| / 256 + 5e-6 max|dx64|"
    else:
        print(f"[{what}] dx: {float(e.max()) / m:.2e} of max|dx64|   (bar 5e-6)")
        assert float(e.max()) <= 5e-6 * m, f"{what}: dx {float(e.max()) / m:.2e}"
    for k, ref in (("dgamma", dg64), ("dbeta", db64)):
        r = float((b[k].to(D64) - ref).abs().max()) / float(ref.abs().max())
        print(f"[{what}] {k}: {r:.2e} of its maximum   (bar 1e-5)")
        assert r <= 1e-5, f"{what}: {k} {r:.2e}"


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_case_vs_fp64(c):
    what = R.case_id(c)
    d = R.case_data(c)
    g = upload(c, d)
    try:
        call("mvd_set_instnorm_small_max", R.small_max_of(c))
        f = twice(lambda: forward(c, g), what)
        check_stats(c, d, f, what)
        if f["y"] is not None:
            check_y(c, d, f, what)
        if c.bwd is not None:
            mean, rstd = up(f["mean"]), up(f["rstd"])
            b = twice(lambda: backward(c, g, mean, rstd), what)
            check_bwd(c, d, b, bwd_mask(c, d, f, what), what)
    finally:
        call("mvd_set_instnorm_small_max", -1)


@pytest.mark.parametrize("xt,yt", R.TYPES)
def test_ops_wrapper_reaches_the_same_entry_points(xt, yt):
    """ops.InstanceNormLeakyReLUFn on the 5-D view (N, C, 1, 1, V) of a case: the bits of the C ABI calls above"""
    c = next(c for c in R.CASES if (c.N, c.V, c.C, c.xt, c.yt, c.entry) == (2, 2431, 320, xt, yt, "norm"))
    d = R.case_data(c)
    g = upload(c, d)
    f = forward(c, g)
    b = backward(c, g, up(f["mean"]), up(f["rstd"]))
    x5 = R.as5d(g["x"]).detach().requires_grad_()
    ga, be = g["gamma"].detach().requires_grad_(), g["beta"].detach().requires_grad_()
    y5 = ops.InstanceNormLeakyReLUFn.apply(x5, ga, be, R.EPS, R.SLOPE, yt == "bf16")
    y5.backward(R.as5d(g["dy"]))
    torch.cuda.synchronize()
    assert y5.dtype == (BF16 if yt == "bf16" else F32) and x5.grad.dtype == g["x"].dtype
    back = lambda t: t.detach().squeeze(2).squeeze(2).permute(0, 2, 1).cpu()  # noqa: E731
    assert torch.equal(back(y5), f["y"]) and torch.equal(back(x5.grad), b["dx"])
    assert torch.equal(ga.grad.cpu(), b["dgamma"]) and torch.equal(be.grad.cpu(), b["dbeta"])


# ------------------------------------------------------------------------------------------------ mean offsets
OFFSETS = (0, 8, 64, 512)
SWEEP = R.Case(2, 8000, 32, "fp32", "fp32", "norm", True, 0, *R.ROWS[("fp32", "fp32")], ())
SWEEP_TILES = R.Case(2, 8000, 32, "fp32", "fp32", "tiles", False, 100, (R.TILES_REDUCE, R.NONE), None, ())


@pytest.mark.parametrize("off", OFFSETS)
def test_mean_offset_sweep(off):
    """mean / std of 0, 8, 64, 512 at V = 8000 <= 8192, C = 32.  rstd: relative error <= 2^-23 (two roundings to float) +
    2^-40 (1 + mean^2 / var), the worst-case cancellation of the fp64 one-pass variance, n 2^-53 at n <= 8192.  y: the fp32
    bar + 2^-24 |mean| rstd max|gamma|, the rounding of the stored float mean.  Synthetic tiles: the same rule, against the
    same rounded tile sums."""
    for c in (SWEEP, SWEEP_TILES):
        d = R.case_data(c, off)
        g = upload(c, d)
        f = forward(c, g)
        ratio = float((d.mean.abs() * d.rstd).max()) ** 2            # mean^2 / (var + eps)
        bar = 2.0 ** -23 + 2.0 ** -40 * (1 + ratio)
        rel = float((f["rstd"].to(D64) / d.rstd - 1).abs().max())
        mrel = float(((f["mean"].to(D64) - d.mean).abs() * d.rstd).max())
        print(f"[offset {off} {c.entry}] rstd {rel:.2e} (bar {bar:.2e})  mean error / std {mrel:.2e}")
        assert rel <= bar, f"offset {off} {c.entry}: rstd {rel:.2e} over {bar:.2e}"
        assert mrel <= 2.0 ** -24 * max(1.0, off) * 1.01 + 2.0 ** -40 * (1 + off), f"offset {off} {c.entry}: mean {mrel:.2e}"
        if f["y"] is not None:
            e = float((f["y"].to(D64) - d.y).abs().max())
            ybar = 2e-6 * max(1.0, float(d.y.abs().max())) + 2.0 ** -24 * float((d.mean.abs() * d.rstd).max()) * float(d.gamma.max())
            print(f"[offset {off} {c.entry}] y {e:.2e} (bar {ybar:.2e})")
            assert e <= ybar, f"offset {off}: y {e:.2e} over {ybar:.2e}"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_host_checks_that_launch_nothing():
    """a misaligned x, y, dy or dx at every entry point, C = 1028, bf16 with C % 4 != 0, a workspace one byte short and
    ntiles == 0: status 2 with a message, and every buffer handed over still holds what it held"""
    lib = _lib.load()
    N, V, C = 2, 2000, 32
    size = N * V * 1028 * 4 + 64
    bufs = {k: torch.full((size if k in ("x", "y", "dy", "dx") else 1 << 20,), 0xA5, dtype=torch.uint8, device=DEV)
            for k in R.POINTERS}
    p = {k: t.data_ptr() for k, t in bufs.items()}
    assert all(a % 16 == 0 for a in p.values())
    wsb = query("mvd_instnorm_workspace_bytes", N, V, C)
    assert wsb == R.workspace_bytes(N, V, C)

    def refused(name, args, match):
        rc = getattr(lib, name)(*args)
        msg = lib.mvd_last_error().decode()
        assert rc == 2 and match in msg, f"{name}: status {rc} ({msg}); wanted the host check '{match}'"

    calls = R.entry_calls(N, V, C, wsb)
    for name, key, which, by in R.misaligned_calls(N, V, C, wsb):
        refused(name, R.bind(p, calls[key][1], which, by), "aligned")
    for name, args in R.entry_calls(N, V, 1028, 1 << 20).values():
        refused(name, R.bind(p, args), "bad shape")
    odd = R.entry_calls(N, V, 30, 1 << 20)
    for key in ("fwd_bf16/x32", "fwd_bf16/x16", "bwd_bf16/x32", "bwd_bf16/x16", "apply_bf16", "stats_bf16"):
        refused(odd[key][0], R.bind(p, odd[key][1]), "C % 4 == 0")
    for key, (name, args) in R.entry_calls(N, V, C, wsb - 1).items():
        if key != "apply_bf16":
            refused(name, R.bind(p, args), "workspace too small")
    name, args = R.entry_calls(N, V, C, wsb, ntiles=0)["prestats"]
    refused(name, R.bind(p, args), "tile statistics required")
    assert lib.mvd_instnorm_stats_from_tiles(p["tiles"], 0, p["mean"], p["rstd"], N, V, C, R.EPS, p["ws"], wsb, None) == 2
    assert lib.mvd_instnorm_finalize_tiles(p["tiles"], 0, p["g"], p["b"], p["mean"], p["rstd"], p["scale"], p["shift"], N, V, C,
                                           R.EPS, None) == 2
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == 0xA5).all()), f"a refused call wrote to {k}"


def test_alignment_is_required_only_where_vectors_are_loaded():
    """C % 4 != 0 runs from a pointer one float off (scalar kernels), a bf16 tensor from an 8-byte boundary that is no 16-byte
    boundary; both give the bits of the aligned call"""
    c = next(c for c in R.CASES if (c.N, c.V, c.C) == (2, 1633, 5))
    d = R.case_data(c)
    g = upload(c, d)
    f = forward(c, g)
    shifted = torch.empty(d.x.numel() + 1, device=DEV)
    shifted[1:] = g["x"].reshape(-1)
    g2 = dict(g, x=shifted[1:])
    assert g2["x"].data_ptr() % 16 == 4
    f2 = forward(c, g2)
    assert all(torch.equal(f[k], f2[k]) for k in ("y", "mean", "rstd"))
    c = next(c for c in R.CASES if (c.N, c.V, c.C, c.xt, c.entry) == (3, 1100, 64, "bf16", "norm"))
    d = R.case_data(c)
    g = upload(c, d)
    f = forward(c, g)
    shifted = torch.empty(d.x.numel() + 4, dtype=BF16, device=DEV)
    shifted[4:] = g["x"].reshape(-1)
    g2 = dict(g, x=shifted[4:])
    assert g2["x"].data_ptr() % 16 == 8
    f2 = forward(c, g2)
    assert all(torch.equal(f[k].view(torch.uint8), f2[k].view(torch.uint8)) for k in ("y", "mean", "rstd"))
