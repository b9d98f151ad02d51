"""CPU tests of the seg-head case table (tests/seghead_ref.py): the library's host-only path queries
(mvd_seghead_fwd_path / _dx_path / _dw_path: the selectors the launch code itself calls, no device call) say which kernel
each case runs.  Every kernel must be reached with every K = 1..8, every case must run the kernels it was written for, and the
thresholds must sit where the table assumes -- so that a later change of a threshold turns this module red instead of
silently un-testing a kernel.  The dispatch does not look at the dtype: the device module runs every case once per entry of
seghead_ref.DTYPES, and the dtype axis of the cells below only pins that this tuple still names both."""
import pytest
import torch

import seghead_ref as S
from multimodal_mvd_seg_amd import _lib

FWD_PATHS, DX_PATHS, DW_PATHS = (0, 1, 2, 4, 8), (0, 1), (0, 1, 2)


def paths(N, V, C, K, aligned=S.ALIGNED):
    lib = _lib.load()
    return (lib.mvd_seghead_fwd_path(N, V, C, K, aligned), lib.mvd_seghead_dx_path(N, V, C, K, aligned),
            lib.mvd_seghead_dw_path(N, V, C, K, aligned))


def cells(cases, dtypes=S.DTYPES):
    """(direction, path, K, dtype) of everything the device module runs over `cases`: it runs each case in both dtypes"""
    got = set()
    for c in cases:
        f, dx, dw = paths(c.N, S.vol(c), c.C, c.K)
        for dt in dtypes:
            got |= {("fwd", f, c.K, dt), ("dx", dx, c.K, dt), ("dw", dw, c.K, dt)}
    return got


def wanted():
    """both input types by name, not from S.DTYPES: taking one out of that tuple empties its cells"""
    return {(d, p, K, dt) for d, ps in (("fwd", FWD_PATHS), ("dx", DX_PATHS), ("dw", DW_PATHS)) for p in ps
            for K in range(1, 9) for dt in ("fp32", "bf16")}


def test_every_kernel_meets_every_class_count_in_both_dtypes():
    missing = wanted() - cells(S.CASES)
    assert not missing, sorted(missing)


def test_coverage_test_notices_an_emptied_cell():
    """the check above is not vacuous: without the cases of any one (direction, path, K) the set is incomplete"""
    for d, ps in (("fwd", FWD_PATHS), ("dx", DX_PATHS), ("dw", DW_PATHS)):
        for p in ps:
            for K in (1, 8):
                kept = [c for c in S.CASES if not (c.K == K and getattr(c, d) == p)]
                assert len(kept) < len(S.CASES)
                assert {(d, p, K, dt) for dt in S.DTYPES} <= wanted() - cells(kept)
    assert wanted() - cells(S.CASES, ("fp32",)) == {w for w in wanted() if w[3] == "bf16"}


@pytest.mark.parametrize("c", S.CASES + (S.BIG_FWD, S.BIG_DX), ids=S.case_id)
def test_case_runs_the_kernels_it_was_written_for(c):
    got = paths(c.N, S.vol(c), c.C, c.K)
    for name, want, g in zip(("forward", "dx", "dw"), (c.fwd, c.dx, c.dw), got):
        assert want is None or g == want, f"{S.case_id(c)}: {name} path {g}, the case declares {want}"


def test_table_has_the_widths_volumes_and_class_counts_it_documents():
    small = {sp for sp, _ in S.SMALL}
    for sp in small:
        for C in S.ALL_C:
            assert {c.K for c in S.CASES if c.sp == sp and c.C == C} == set(range(1, 9)), (sp, C)
    assert {c.N for c in S.CASES if c.sp in small} == {1, 3}
    for N, sp, quads, cs, _ in S.LARGER:
        assert (sp[0] * sp[1] * sp[2] % 4 == 0) == quads
        for C in cs:
            assert {c.K for c in S.CASES if (c.N, c.sp, c.C) == (N, sp, C)} == set(S.K_LARGER)
    for sp, quads in S.SMALL:
        assert (sp[0] * sp[1] * sp[2] % 4 == 0) == quads
    assert len(set(S.CASES)) == len(S.CASES) and len({S.case_id(c) for c in S.CASES}) == len(S.CASES)


def test_weight_gradient_block_counts_are_the_documented_ones():
    """nblk of the weight-gradient pass from the workspace size the library asks for: nblk (K C + K) doubles + 256 bytes"""
    lib = _lib.load()
    for N, sp, _, cs, nblk in S.LARGER:
        V = sp[0] * sp[1] * sp[2]
        for C in cs:
            for K in S.K_LARGER:
                nbytes = lib.mvd_seghead_bwd_workspace_bytes(N, V, C, K)
                assert (nbytes - 256) == nblk * (K * C + K) * 8, (N, sp, C, K, (nbytes - 256) / ((K * C + K) * 8))


def test_thresholds_sit_where_the_code_says():
    A = S.ALIGNED
    # forward: 2 / 4 / 8 lanes per voxel below 2^20 voxels in the batch, one thread per voxel from there on
    assert paths(1, (1 << 20) - 1, 64, 3)[0] == 2 and paths(1, 1 << 20, 64, 3)[0] == 1
    assert paths(2, (1 << 19) - 1, 320, 5)[0] == 8 and paths(2, 1 << 19, 320, 5)[0] == 1
    assert [paths(1, 64, C, 5)[0] for C in (32, 64, 96, 127, 128, 224, 255, 256, 288, 320, 1024, 1028)] == \
        [1, 2, 2, 0, 4, 4, 0, 8, 8, 8, 8, 1]
    assert [paths(1, 64, C, 5)[0] for C in (1, 2, 3, 4, 5, 8, 30, 36)] == [0, 0, 0, 1, 0, 1, 0, 1]
    # dx: 4-channel groups up to one 256-lane row, quads of voxels
    assert paths(1, 8, 1024, 8)[1] == 1 and paths(1, 8, 1028, 8)[1] == 0
    assert paths(1, 8, 32, 8)[1] == 1 and paths(1, 7, 32, 8)[1] == 0 and paths(1, 8, 33, 8)[1] == 0
    # dw: V % 4 picks between dw4v and dw4; C beyond one row or no multiple of 4 is generic
    assert paths(1, 240, 32, 5)[2] == 2 and paths(1, 315, 32, 5)[2] == 1
    assert paths(5, 8, 1024, 8)[2] == 2 and paths(5, 8, 1028, 8)[2] == 0 and paths(5, 8, 70, 8)[2] == 0
    # alignment: a misaligned x gives the generic forward and the generic dw, and leaves dx alone
    for C in (32, 64, 320):
        assert paths(1, 240, C, 5, A & ~S.AL_X) == (0, 1, 0)
    assert paths(1, 240, 64, 5, A & ~S.AL_W) == (1, 0, 2)        # voxp and dx4 read w as float4
    assert paths(1, 240, 64, 5, A & ~S.AL_DL) == (2, 0, 1)       # dx4 and dw4v read dlogits as float4
    assert paths(1, 240, 64, 5, A & ~S.AL_DX) == (2, 0, 2)
    # the class count decides nothing but validity
    for K in range(1, 9):
        assert paths(3, 240, 64, K) == (2, 1, 2) and paths(3, 315, 33, K) == (0, 0, 0)


def test_queries_refuse_what_the_entry_points_refuse():
    for bad in ((1, 64, 32, 0), (1, 64, 32, 9), (0, 64, 32, 5), (65536, 64, 32, 5), (1, 0, 32, 5), (1, 64, 0, 5)):
        assert paths(*bad) == (-1, -1, -1), bad
    assert paths(65535, 1, 32, 8) == (1, 0, 1)


def test_integer_data_of_a_case_is_exact_and_bounded():
    """the integer reference is the same whether summed in fp64 or in fp32 (what 'exact in any order' rests on), and dx fits
    bf16"""
    c = next(c for c in S.CASES if c.C == 1028 and c.K == 8 and c.sp == (5, 7, 9))
    (x, w, b, dl), (y, dx, dw, db) = S.integer_case(c)
    assert x.is_contiguous(memory_format=torch.channels_last_3d)
    y32 = torch.einsum('kc,ncdhw->nkdhw', w.view(c.K, c.C), x) + b.view(1, -1, 1, 1, 1)
    assert torch.equal(y32, y) and float(y.abs().max()) > 100
    assert torch.equal(dx.to(S.BF16).float(), dx) and float(dx.abs().max()) <= 2 * c.K
    assert torch.equal(torch.einsum('nkdhw,ncdhw->kc', dl, x).view_as(dw), dw)
