"""The dispatcher rule of mvd_conv3d_fwd_routed / mvd_conv3d_dgrad_routed: given a table of kind E, engine E runs if and only
if E's predicate holds for the pass; otherwise the direct engines run, with the result of mvd_conv3d_fwd / mvd_conv3d_dgrad
bit for bit.  The table is all zeros, so a call that runs the Winograd engine returns the bias alone (the forward) or zero
(the input gradient) and a call that falls back returns the convolution: which engine ran cannot be mistaken.  Smallest
shapes: N = 1, 32 -> 32 channels, 8x8x8 for the 3x3x3 engines and 4x8x16 for the in-plane one."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SETTERS = ("mvd_set_wino_min_items", "mvd_set_wino3_min_items", "mvd_set_wino2p_min_items")
# kind name -> (kernel size, volume, applicability query, table-size query, the minimum that turns the predicate off)
CASES = {
    "CONV_WINO2": ((3, 3, 3), (8, 8, 8), "mvd_conv_wino_applicable", "mvd_wino_weight_elems", "mvd_set_wino_min_items"),
    "CONV_WINO3": ((3, 3, 3), (8, 8, 8), "mvd_conv_wino3_applicable", "mvd_wino3_weight_elems", "mvd_set_wino3_min_items"),
    "CONV_WINO2P": ((1, 3, 3), (4, 8, 16), "mvd_conv_wino2p_applicable", "mvd_wino2p_weight_elems", "mvd_set_wino2p_min_items"),
}


@pytest.mark.parametrize("kind_name", list(CASES))
def test_table_engine_runs_iff_its_predicate_holds(kind_name):
    from multimodal_mvd_seg_amd import _lib, ops
    from multimodal_mvd_seg_amd._lib import call, i3, query
    ks, sp, applicable, elems, off_switch = CASES[kind_name]
    kind = getattr(_lib, kind_name)
    N, C, K = 1, 32, 32
    D, H, W = sp
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    shape = (N, D, H, W, C, 0, K, i3(ks), i3((1, 1, 1)))
    try:
        for fn in SETTERS:
            call(fn, 1)
        if query(applicable, *shape) != 3:
            pytest.skip("this engine is switched off for this run (MVD_WINO / MVD_WINO3)")
        g = torch.Generator().manual_seed(7)
        x = ops.to_ndhwc(torch.randn(N, C, D, H, W, generator=g).to(DEV))
        dy = ops.to_ndhwc(torch.randn(N, K, D, H, W, generator=g).to(DEV))
        w = (torch.randn(K, C, *ks, generator=g) * 0.1).to(DEV)
        b = torch.randn(K, generator=g).to(DEV)
        wf, wb = ops.pack_weight(w, False)
        zero = torch.zeros(query(elems, C, K), device=DEV)
        ws = torch.empty(max(query("mvd_conv_fwd_workspace_bytes", N, D * H * W, max(C, K)), 1024), dtype=torch.uint8, device=DEV)

        def fwd(table, k):
            y = ops.empty_cl3d((N, K, D, H, W), DEV).fill_(float("nan"))
            call("mvd_conv3d_fwd_routed", P(x), C, None, 0, P(wf), P(table) if table is not None else None, k, P(b), P(y), None, 0,
                 None, N, D, H, W, K, i3(ks), i3((1, 1, 1)), P(ws), ws.numel(), s)
            return y

        def dgrad(table, k):
            dx = ops.empty_cl3d((N, C, D, H, W), DEV).fill_(float("nan"))
            call("mvd_conv3d_dgrad_routed", P(dy), P(wb), P(table) if table is not None else None, k, P(dx), C, None, 0, N, D, H, W,
                 K, i3(ks), i3((1, 1, 1)), P(ws), ws.numel(), s)
            return dx

        y_direct, dx_direct = fwd(None, _lib.CONV_DIRECT), dgrad(None, _lib.CONV_DIRECT)
        assert float(y_direct.std()) > 0.1 and float(dx_direct.std()) > 0.1
        # predicate holds: the table's engine runs (the zero table shows)
        assert query("mvd_conv3d_route", *shape) in (kind | kind << 4, _lib.CONV_WINO3 | _lib.CONV_WINO3 << 4)
        y_engine, dx_engine = fwd(zero, kind), dgrad(zero, kind)
        assert torch.equal(y_engine, b.view(1, K, 1, 1, 1).expand_as(y_engine))
        assert torch.equal(dx_engine, torch.zeros_like(dx_engine))
        # predicate fails (work items below the minimum): the same call falls back to the direct engines
        call(off_switch, 1 << 40)
        assert query(applicable, *shape) == 0
        y_fall, dx_fall = fwd(zero, kind), dgrad(zero, kind)
        torch.cuda.synchronize()
        assert torch.equal(y_fall, y_direct)
        assert torch.equal(dx_fall, dx_direct)
    finally:
        for fn in SETTERS:
            call(fn, -1)
