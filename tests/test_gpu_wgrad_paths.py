"""Every weight-gradient kernel path of wgrad_plan (csrc/conv_mfma.hip) against fp64 at its dispatch edges: the case table of
tests/wgrad_ref.py (tests/test_wgrad_cases_host.py checks on the CPU which kernel and which edges each case reaches), called
through the C ABI -- mvd_conv3d_wgrad, mvd_convT3d_wgrad and their bf16 twins -- so that the test owns every buffer.

  * workspace: exactly the size the query returns, 0xFF bytes before every call -- a split-K partial or a bias row that no
    workgroup wrote reads as NaN -- and a guard tail that must still hold 0xFF afterwards;
  * dw, dbias: filled with a NaN sentinel and allocated with a guard tail: the tail must still hold the sentinel after the
    call, no element inside may;
  * which kernel ran: mvd_conv_wgrad_last_kernel() (a host store beside the launch) equals the kernel of the plan, and
    mvd_wgrad_wino3_launches moves by one exactly where the plan says k_wgrad_wino3;
  * reference: torch.nn.functional.conv3d / conv_transpose3d backward in fp64 on the CPU on the same operands (bf16: the
    bf16-rounded operands);
  * bars, the project's own: max|dw - dw64| <= 2e-5 max|dw64| (tests/test_gpu_parity.py, close_f32 of tests/test_gpu_bf16.py),
    relative L2 of dw <= 1e-5 and max|db - db64| <= 2e-6 max_k sum|dy| + 1e-12 (tests/test_gpu_wgrad_bias_fold.py); dy has
    mean 0.25 so the bias gradient is a real sum;
  * exact integer data (x in -2..2, dy in -1..1): dw and dbias must equal the exact result bit for bit, for every kernel.
    The direct kernels only add products of small integers in fp32.  The three Winograd kernels are held to the same: their
    input transforms (B^T d B, rows of 0, +1, -1) and dy transforms (sums of two values per axis) turn small integers into
    small integers -- at most 16 |x| and 8 |dy| in 3-D -- the fp32 MFMA sums integer products far below 2^24, and the output
    transform (G^T M G, entries 1, +-1/2) runs in the reduce kernels in fp64 on those integers, where halves and quarters are
    exact; the result is the integer dW itself.  No scaling by a power of two is needed;
  * every evaluation runs twice and must repeat bit for bit; setters are restored in `finally`.
Cases under MVD_WINO=1 (k_wgrad_wino) run in one fresh child process, which executes this module's own checks.

Measured on an MI355X, the worst case of the table per kernel on random data (max|dw - dw64| / max|dw64|, bar 2e-5; relative
L2 of dw, bar 1e-5; max|db - db64| as a fraction of its bar); integer data exact and run-to-run identical for every case:
    k_wgrad_wino3     2.5e-07  2.2e-07  0.022        k_wgrad16       1.1e-07  8.3e-08  0.011
    k_wgrad_wino2w12  3.4e-07  1.7e-07  0.026        k_wgrad16z      6.6e-07  3.6e-07  0.025
    k_wgrad_wino      3.8e-07  1.7e-07  0.013        k_wgrad16zs     2.9e-07  1.7e-07  0.009
    k_wgrad_smallc    3.2e-07  2.8e-07  0.027        k_wgrad_scalar  6.7e-08  3.7e-08  0.021
    k_wgrad_mfma      1.6e-07  1.1e-07  0.026
No case needed a smaller shape or a derived bar."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as R
from multimodal_mvd_seg_amd import _lib
from multimodal_mvd_seg_amd._lib import call, query

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(R.skip_reason() is not None, reason=str(R.skip_reason()))]
D64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32
GUARD = 1024                 # elements behind dw and dbias, bytes x 4 behind the workspace
NAN32 = 0x7FC0DEAD           # a quiet NaN (as an int32 bit pattern) no kernel produces


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Out:
    """an fp32 output of `shape` with a guard tail, everything filled with a NaN sentinel"""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.n, self.shape = n, tuple(shape)
        self.raw = torch.full((n + GUARD,), NAN32, dtype=torch.int32, device=_dev())
        assert self.raw.data_ptr() % 16 == 0

    def take(self, what):
        raw = self.raw.cpu()
        assert bool((raw[self.n:] == NAN32).all()), f"{what}: written past its end"
        left = int((raw[:self.n] == NAN32).sum())
        assert left == 0, f"{what}: {left} of {self.n} elements were not written"
        return raw[:self.n].view(F32).reshape(self.shape)


def operands(c, integer):
    """x1, x2 [N, D, H, W, C] and dy [N, Do, Ho, Wo, K] on the host in fp32 (bf16 cases: already rounded to bf16)"""
    g = torch.Generator().manual_seed(1000 * c.C1 + 10 * c.K + c.sp[2] + (7 if integer else 0))
    osp = R.out_sp(c)

    def draw(shape, lo, hi, mean):
        if integer:
            return torch.randint(lo, hi + 1, shape, generator=g).to(F32)
        t = torch.randn(shape, generator=g) + mean
        return t.to(BF16).to(F32) if c.dt == "bf16" else t

    x1 = draw((c.N, *c.sp, c.C1), -2, 2, 0.0)
    x2 = draw((c.N, *c.sp, c.C2), -2, 2, 0.0) if c.C2 else None
    dy = draw((c.N, *osp, c.K), -1, 1, 0.25)
    return x1, x2, dy


def reference(c, x1, x2, dy):
    """dw (torch layout) and dbias in fp64 from the backward of torch's own convolution"""
    x = torch.cat([x1] + ([x2] if x2 is not None else []), -1).to(D64).permute(0, 4, 1, 2, 3)
    gy = dy.to(D64).permute(0, 4, 1, 2, 3)
    b = torch.zeros(c.K, dtype=D64, requires_grad=True)
    if c.kind == "conv":
        w = torch.zeros(c.K, c.C1 + c.C2, *c.ks, dtype=D64, requires_grad=True)
        y = F.conv3d(x, w, b, c.st, tuple((k - 1) // 2 for k in c.ks))
    else:
        w = torch.zeros(c.C1, c.K, *c.st, dtype=D64, requires_grad=True)
        y = F.conv_transpose3d(x, w, b, c.st)
    assert tuple(y.shape) == tuple(gy.shape)
    y.backward(gy)
    return w.grad.reshape(w.shape[0], w.shape[1], -1), b.grad


def run(c, p, x1, x2, dy):
    """one call of the case's entry point on buffers the test owns: (dw, dbias or None) on the host"""
    dev, bf = _dev(), c.dt == "bf16"
    up = lambda t: None if t is None else (t.to(BF16) if bf else t).contiguous().to(dev)
    d1, d2, dg = up(x1), up(x2), up(dy)
    assert all(t is None or t.data_ptr() % 16 == 0 for t in (d1, d2, dg))
    T, Cs = R.ntaps(c), c.C1 + c.C2
    dw = Out((c.K, Cs, T) if c.kind == "conv" else (c.C1, c.K, T))
    db = Out((c.K,)) if c.bias else None
    nws = R.workspace_bytes(c)
    assert nws == p.ws_bytes
    ws = torch.full((nws + 4 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w3 = query("mvd_wgrad_wino3_launches")
    sfx = "_bf16" if bf else ""
    if c.kind == "conv":
        call("mvd_conv3d_wgrad" + sfx, _p(d1), c.C1, _p(d2), c.C2, _p(dg), _p(dw.raw), _p(db.raw) if db else None, c.N, *c.sp,
             c.K, _lib.i3(c.ks), _lib.i3(c.st), _p(ws), nws, stream)
    else:
        call("mvd_convT3d_wgrad" + sfx, _p(d1), _p(dg), _p(dw.raw), _p(db.raw) if db else None, c.N, *c.sp, c.C1, c.K,
             _lib.i3(c.st), _p(ws), nws, stream)
    torch.cuda.synchronize()
    ran = query("mvd_conv_wgrad_last_kernel")
    assert ran == p.kernel, f"ran {R.KERNEL_NAMES[ran]}, planned {R.KERNEL_NAMES[p.kernel]}"
    assert query("mvd_wgrad_wino3_launches") - w3 == (1 if p.kernel == R.WINO3 else 0)
    assert bool((ws[nws:] == 0xFF).all()), "workspace: written past its end"
    return dw.take("dw"), (db.take("dbias") if db else None)


def check_case(c):
    """both data sets of a case, each evaluated twice; returns the measured figures"""
    with R.applied(c):
        p = R.raw_plan(c.kind == "convT", c.dt == "bf16", c.N, c.sp, c.C1, c.C2, c.K, c.ks, c.st, 0, c.bias)
        assert p is not None and p.kernel == c.kernel, f"planned {p}, the case declares {R.KERNEL_NAMES[c.kernel]}"
        out = {}
        for integer in (False, True):
            x1, x2, dy = operands(c, integer)
            dw, db = run(c, p, x1, x2, dy)
            dw2, db2 = run(c, p, x1, x2, dy)
            assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), "run-to-run"
            dw64, db64 = reference(c, x1, x2, dy)
            if integer:
                bad = int((dw != dw64.to(F32)).sum())
                assert bad == 0, f"integer data: {bad} of {dw.numel()} dw values are not the exact result"
                assert db is None or torch.equal(db, db64.to(F32)), "integer data: dbias is not the exact sum"
                continue
            e = (dw.to(D64) - dw64)
            out["dw_max"] = float(e.abs().max() / dw64.abs().max())
            out["dw_l2"] = float(e.norm() / dw64.norm())
            print(f"[{R.case_id(c)}] {R.KERNEL_NAMES[p.kernel]}: dw max {out['dw_max']:.2e} (bar 2e-5) L2 {out['dw_l2']:.2e} (bar 1e-5)",
                  end="")
            if db is not None:
                tol = 2e-6 * float(dy.to(D64).abs().sum((0, 1, 2, 3)).max()) + 1e-12
                out["db"] = float((db.to(D64) - db64).abs().max()) / tol
                print(f" db {out['db']:.2e} of its bar", end="")
            print()
            assert out["dw_max"] <= 2e-5, f"max|dw - dw64| = {out['dw_max']:.2e} max|dw64|"
            assert out["dw_l2"] <= 1e-5, f"relative L2 error of dw {out['dw_l2']:.2e}"
            assert db is None or out["db"] <= 1.0, f"max|db - db64| is {out['db']:.2f} of 2e-6 max_k sum|dy|"
        return out


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    yield
    for name, default in R.SETTERS.values():
        call(name, default)


@pytest.mark.parametrize("c", [c for c in R.CASES if not c.env], ids=R.case_id)
def test_case_against_fp64(c):
    check_case(c)


def test_cases_under_mvd_wino_1_in_one_child_process():
    """k_wgrad_wino exists only under MVD_WINO=1, read at process start: all its cases in one fresh process"""
    todo = [c for c in R.CASES if c.env]
    assert todo and all(c.env == (("MVD_WINO", "1"),) for c in todo)
    from conftest import ROOT
    env = dict(os.environ, MVD_WINO="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    done = json.loads(r.stdout.strip().splitlines()[-1])
    assert done == [R.case_id(c) for c in todo]


if __name__ == "__main__":   # the child of the test above
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _lib.load()
    assert query("mvd_wino_mode") == 1
    ids = []
    for case in R.CASES:
        if case.env == (("MVD_WINO", "1"),):
            check_case(case)
            ids.append(R.case_id(case))
    print(json.dumps(ids))
