"""CPU tests of the InstanceNorm case table (tests/instnorm_ref.py).  The library's host-only plan query
(mvd_instnorm_plan: the function the launch code itself consumes, no device call) says which kernels an entry point runs and
on which grids.  The Python restatement must equal it on a grid around every threshold; every case must run the kernels and sit
in the geometry classes it declares; and every cell (kernel x geometry class it can meet x type combination) must have a case
-- so that a later change of a threshold turns this module red instead of silently un-testing a path.  The refusals of the
entry points are host checks in front of any launch: they are exercised here with pointers that are never dereferenced."""
import ctypes

import pytest

import instnorm_ref as R
from multimodal_mvd_seg_amd import _lib

F32, F16, B16 = ("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "bf16")
NS = ("N=1", "N=2", "N=3", "N>2048")
REGIMES = ("nblk=1", "nblk=2..64", "nblk=65..128", "nblk>128")
EDGES = ("idle_lanes", "R=1", "R=256")
REM4 = ("rem0", "rem1", "rem2", "rem3")
NTILES = ("ntiles<64", "ntiles=64..255", "ntiles>=256", "ntiles>=256,%64")
# kernel -> (the geometry classes it can meet, the type combinations it runs in)
MATRIX = {
    "stats4": (REGIMES + ("ragged_stats", "empty_block") + REM4 + EDGES + NS, (F32, F16, B16)),
    "bwd_stats4": (REGIMES + ("ragged_stats", "empty_block", "rem0", "rem1") + EDGES + NS, (F32, F16, B16)),
    "apply_rows": (("ragged_apply",) + REM4 + EDGES + NS, (F32, F16)),
    "apply_ss16": (("ragged_apply",) + REM4 + EDGES + NS, (B16,)),
    "bwd_apply_rows": (("ragged_apply",) + REM4 + EDGES + NS, (F32, F16, B16)),
    "stats1": (REGIMES + ("ragged_stats", "empty_block") + EDGES + NS, (F32,)),
    "bwd_stats1": (REGIMES + ("ragged_stats", "empty_block") + EDGES + NS, (F32,)),
    "apply1": (("any", "grid_stride") + NS, (F32,)),
    "bwd_apply1": (("any", "grid_stride") + NS, (F32,)),
    "tiles_reduce": (NTILES + ("C<256", "C=256", "C>256", "cap_64", "cap_nblk", "uncapped", "nblk=1", "nblk=2..64") + REM4, (F32,)),
    "finalize_tiles": (NTILES + REM4, (B16,)),
    "small_fwd": (("any",), (F32,)), "small_bwd": (("any",), (F32,)),
    "bwd_stats_head": (("any", "ragged_stats", "empty_block"), (F32,)), "bwd_apply_head": (("any", "ragged_apply"), (F32,)),
}


@pytest.fixture(autouse=True)
def _restore_small_max():
    yield
    _lib.load().mvd_set_instnorm_small_max(-1)


def lib_plan(d, N, V, C, xb, yb, ntiles=0, head=0, small_max=R.SMALL_MAX_DEFAULT):
    lib = _lib.load()
    lib.mvd_set_instnorm_small_max(small_max)
    buf = (ctypes.c_long * R.PLAN_LEN)()
    rc = lib.mvd_instnorm_plan(d, N, V, C, int(xb), int(yb), ntiles, int(head), buf)
    assert rc in (0, 2) and (rc == 0 or len(lib.mvd_last_error()) > 10)
    return R.Plan(*buf) if rc == 0 else None


def cells(cases):
    """(kernel, geometry class, x type, y type) of everything the device module runs over `cases`, from the LIBRARY's plans"""
    got = set()
    for c in cases:
        for d in (0, 1) if c.bwd else (0,):
            p = lib_plan(d, *R.plan_args(c, d), small_max=R.small_max_of(c))
            got |= {(R.KERNEL_NAMES[k], cl, c.xt, c.yt) for k, cl in R.classes(p, c.N, c.V, c.C, c.ntiles)}
    return got


def wanted():
    return {(k, cl, *t) for k, (cls, types) in MATRIX.items() for cl in cls for t in types}


def test_matrix_names_every_kernel_of_the_header():
    assert set(MATRIX) == set(R.KERNEL_NAMES[1:])
    import os
    import re
    from conftest import ROOT
    ids = dict(re.findall(r"#define MVD_IN_(\w+) (\d+)", open(os.path.join(ROOT, "include", "mvdseg_hip.h")).read()))
    assert int(ids.pop("PLAN_LEN")) == R.PLAN_LEN
    assert {n.lower(): int(v) for n, v in ids.items()} == {n: i for i, n in enumerate(R.KERNEL_NAMES)}


def test_every_cell_of_the_matrix_has_a_case():
    missing = wanted() - cells(R.CASES)
    assert not missing, sorted(missing)


def test_coverage_test_notices_an_emptied_cell():
    """the check above is not vacuous: without the cases that sit in a cell, that cell is missing"""
    per_case = {c: cells((c,)) for c in R.CASES}
    for cell in sorted(wanted()):
        kept = [c for c in R.CASES if cell not in per_case[c]]
        assert len(kept) < len(R.CASES), cell
        assert cell not in set().union(*(per_case[c] for c in kept)), cell


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_case_runs_the_kernels_and_sits_in_the_classes_it_declares(c):
    assert c.N * c.V * c.C * 4 <= 11 << 20, "a tensor of a case is at most about 10 MB"
    names = set()
    for d, want in ((0, c.fwd), (1, c.bwd)):
        if want is None:
            continue
        p = lib_plan(d, *R.plan_args(c, d), small_max=R.small_max_of(c))
        assert p is not None and (p.stats, p.apply) == want, f"{R.case_id(c)}: direction {d} runs {p}, the case declares {want}"
        assert p == R.plan(d, *R.plan_args(c, d), small_max=R.small_max_of(c))
        names |= {cl for _, cl in R.classes(p, c.N, c.V, c.C, c.ntiles)}
    assert set(c.why) <= names, f"{R.case_id(c)}: declared {set(c.why) - names}, the plan gives {sorted(names)}"
    if c.ntiles:
        assert sum(R.tile_sizes(c.V, c.ntiles)) == c.V


def test_table_has_the_widths_and_batches_the_issue_lists():
    norm = [c for c in R.CASES if c.entry == "norm"]
    assert {4, 32, 36, 64, 96, 128, 256, 320, 512, 1024} <= {c.C for c in norm if c.C % 4 == 0}
    assert {1, 5, 30, 257, 1022} <= {c.C for c in norm if c.C % 4}
    assert {1, 2, 3, 2049} <= {c.N for c in norm}
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    for t in R.TYPES:
        assert {(c.N, c.V, c.C) for c in norm if (c.xt, c.yt) == t and c.C % 4 == 0 and c.fwd[0] == R.STATS4} == \
            {s[:3] for s in R.ROW_SHAPES}


def _grid():
    for C in (1, 4, 5, 30, 32, 36, 64, 96, 128, 252, 256, 257, 260, 320, 512, 1020, 1022, 1023, 1024):
        R_ = R.norm_geom(1, 1, C)[1]
        vs = {1, 2, 255, 256, 257, 1023, 1024, 1025, 2431, 70001, R.SMALL_MAX_DEFAULT // C, R.SMALL_MAX_DEFAULT // C + 1}
        for k in (1, 2, 64, 65, 128, 129):          # blocks of the statistics pass (16 R voxels) and the apply pass (8 R)
            vs |= {k * m * R_ + e for m in (8, 16) for e in (-1, 0, 1)}
        for V in sorted(v for v in vs if v > 0):
            for N in (1, 2, 3, 4, 5, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 65535):
                if N * V * C <= 1 << 34:
                    yield N, V, C


def test_restatement_equals_the_librarys_plan_around_every_threshold():
    n = 0
    for N, V, C in _grid():
        for xb, yb in ((0, 0), (0, 1), (1, 1), (1, 0)):
            for sm in (R.SMALL_MAX_DEFAULT, 0) if not (xb or yb) else (0,):
                for d, nt, head in ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)):
                    got, want = lib_plan(d, N, V, C, xb, yb, nt, head, sm), R.plan(d, N, V, C, xb, yb, nt, head, sm)
                    assert got == want, (d, N, V, C, xb, yb, nt, head, sm, got, want)
                    n += 1
        if N in (1, 2, 1025, 2049):
            for nt in (1, 63, 64, 65, 255, 256, 257, 4096, 4097, 9000):
                for xb, yb, head in ((0, 0, 0), (0, 0, 1), (1, 1, 0), (0, 1, 0), (1, 1, 1)):
                    got, want = lib_plan(0, N, V, C, xb, yb, nt, head, 0), R.plan(0, N, V, C, xb, yb, nt, head, 0)
                    assert got == want, (N, V, C, xb, yb, nt, head, got, want)
                    n += 1
    assert n > 20000


def test_thresholds_sit_where_the_table_assumes():
    P = lib_plan
    # statistics blocks: one per 16 R voxels, at most 2048 / N
    assert (P(0, 1, 511, 32, 0, 1).nblk, P(0, 1, 1023, 32, 0, 1).nblk, P(0, 1, 1024, 32, 0, 1).nblk) == (1, 1, 2)
    assert (P(0, 2048, 4096, 32, 0, 1).nblk, P(0, 1025, 4096, 32, 0, 1).nblk, P(0, 1024, 4096, 32, 0, 1).nblk) == (1, 1, 2)
    assert P(0, 1, 700, 1024, 0, 0)[5:7] == (43, 17) and P(0, 1, 700, 1022, 0, 0)[5:7] == (43, 17)  # block 42 is empty
    assert P(0, 2, 2431, 320, 0, 0)[2:9] == (256, 3, 80, 50, 49, 98, 25)
    assert P(0, 2, 1633, 5, 0, 0)[2:7] == (256, 51, 5, 2, 817) and P(0, 2, 300, 257, 0, 0)[2:5] == (320, 1, 257)
    assert P(0, 1, 70001, 1, 0, 0).R == 256 and P(0, 1, 70001, 4, 0, 0).R == 256 and P(0, 1, 700, 1022, 0, 0).threads == 1024
    # apply blocks: one per 8 R voxels, at most 8192 / N; the scalar form: 256 elements per block, at most 4096 / N
    assert P(0, 8192, 4096, 32, 0, 1).agrid == 1 and P(0, 4096, 4096, 32, 0, 1).agrid == 2
    assert P(0, 1, 1200, 1022, 0, 0).agrid == 4096 and P(0, 1, 1000, 1022, 0, 0).agrid == 3993
    # the single launch: V <= 1024 and V C at most the limit (the backward: 2 / N of it past two samples)
    assert P(0, 2, 1024, 320, 0, 0).stats == R.SMALL_FWD and P(0, 2, 1024, 324, 0, 0).stats == R.STATS4
    assert P(0, 2, 1025, 32, 0, 0).stats == R.STATS4 and P(0, 2, 1024, 32, 0, 0, small_max=0).stats == R.STATS4
    assert P(1, 4, 500, 32, 0, 0, small_max=32000).stats == R.SMALL_BWD and P(1, 5, 500, 32, 0, 0, small_max=32000).stats == R.BWD_STATS4
    assert P(0, 2, 512, 32, 0, 1).stats == R.STATS4 and P(0, 2, 512, 32, 0, 0, 9).stats == R.SMALL_FWD  # prestats: tiles not needed
    # tiles: a block per 64 tiles, at most 64 and at most the statistics blocks the workspace was sized for
    assert P(0, 1, 33000, 32, 0, 0, 4096, 0, 0)[9:11] == (64, 64) and P(0, 1, 33000, 32, 0, 0, 4097, 0, 0)[9:11] == (64, 65)
    assert P(0, 2, 1500, 32, 0, 0, 200, 0, 0)[9:13] == (2, 100, 32, 8) and P(0, 1, 6000, 320, 0, 0, 333, 0, 0)[9:13] == (6, 56, 256, 1)
    assert P(0, 1, 9000, 320, 1, 1, 333).stats == R.FINALIZE_TILES and P(0, 1, 9000, 320, 0, 0, 333, 1).apply == R.NONE
    # the type decides the apply kernel of the forward and nothing else
    assert [P(0, 2, 2431, 320, *t).apply for t in ((0, 0), (0, 1), (1, 1))] == [R.APPLY_ROWS, R.APPLY_ROWS, R.APPLY_SS16]
    assert len({P(1, 2, 2431, 320, *t) for t in ((0, 0), (0, 1), (1, 1))}) == 1


def test_plan_refuses_what_the_entry_points_refuse():
    for bad in ((0, 0, 64, 32, 0, 0), (0, 65536, 64, 32, 0, 0), (0, 1, 0, 32, 0, 0), (0, 1, 64, 0, 0, 0), (0, 1, 64, 1028, 0, 0),
                (2, 1, 64, 32, 0, 0), (0, 1, 64, 30, 0, 1), (1, 1, 64, 30, 1, 1), (0, 1, 64, 32, 1, 0), (1, 1, 64, 32, 1, 0),
                (1, 1, 64, 32, 0, 0, 5), (0, 1, 64, 32, 0, 0, -1), (1, 1, 64, 30, 0, 0, 0, 1), (1, 1, 64, 32, 0, 1, 0, 1),
                (0, 1, 64, 32, 0, 1, 7), (0, 1, 64, 30, 0, 0, 0, 1), (0, 1, 64, 32, 1, 1, 7, 1)):
        assert lib_plan(*bad) is None and R.plan(*(list(bad) + [0, 0])[:8]) is None, bad
    assert lib_plan(0, 65535, 1, 1024, 1, 1) is not None and lib_plan(1, 1, 64, 1024, 0, 0, 0, 1) is not None
    assert _lib.load().mvd_instnorm_plan(0, 1, 64, 32, 0, 0, 0, 0, None) == 2


# ------------------------------------------------------------------------------------------------ refusals of the entry points
BASE = 1 << 20  # a 16-byte aligned address that is never dereferenced: every call below must return before any launch


def _entry_calls(N, V, C, ws_bytes, ntiles=5):
    return {k: BASE + 4096 * i for i, k in enumerate(R.POINTERS)}, R.entry_calls(N, V, C, ws_bytes, ntiles)


_args = R.bind


def _refused(name, *args, match):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.mvd_last_error().decode()
    assert rc == 2 and match in msg, f"{name}: status {rc} ({msg}); wanted the host check '{match}'"


def test_entry_points_refuse_a_misaligned_tensor_before_any_launch():
    """x, y, dy and dx offset by one element (4 bytes fp32, 2 bytes bf16): status 2 and the alignment message"""
    N, V, C = 2, 2000, 32
    p, calls = _entry_calls(N, V, C, R.workspace_bytes(N, V, C))
    todo = R.misaligned_calls(N, V, C, R.workspace_bytes(N, V, C))
    assert len(todo) == 22 and {n for n, _, _, _ in todo} == {n for n, _ in calls.values()}
    for name, key, which, by in todo:
        _refused(name, *_args(p, calls[key][1], which, by), match="aligned")
    # a bf16 tensor on an 8-byte boundary that is no 16-byte boundary is accepted by the check: nothing to refuse, nothing run
    # here; C % 4 != 0 has no vector access and no requirement (tests/test_gpu_instnorm_paths.py runs both)


def test_entry_points_refuse_bad_shapes_types_and_workspaces_before_any_launch():
    N, V = 2, 2000
    p, calls = _entry_calls(N, V, 1028, 1 << 30)
    for key, (name, args) in calls.items():
        _refused(name, *_args(p, args), match="bad shape")
    p, calls = _entry_calls(N, V, 30, 1 << 30)
    for key in ("fwd_bf16/x32", "fwd_bf16/x16", "bwd_bf16/x32", "bwd_bf16/x16", "apply_bf16"):
        _refused(calls[key][0], *_args(p, calls[key][1]), match="C % 4 == 0")
    _refused(calls["stats_bf16"][0], *_args(p, calls["stats_bf16"][1]), match="C % 4 == 0")
    _refused(calls["bwd_head"][0], *_args(p, calls["bwd_head"][1]), match="logit-gradient form")
    p, calls = _entry_calls(N, V, 32, R.workspace_bytes(N, V, 32) - 1)
    for key, (name, args) in calls.items():
        if key != "apply_bf16":
            _refused(name, *_args(p, args), match="workspace too small")
    p, calls = _entry_calls(N, V, 32, 1 << 30, ntiles=0)
    _refused(calls["prestats"][0], *_args(p, calls["prestats"][1]), match="tile statistics required")
    lib = _lib.load()
    assert lib.mvd_instnorm_stats_from_tiles(p["tiles"], 0, p["mean"], p["rstd"], N, V, 32, R.EPS, p["ws"], 1 << 30, None) == 2
    assert lib.mvd_instnorm_finalize_tiles(p["tiles"], 0, p["g"], p["b"], p["mean"], p["rstd"], p["scale"], p["shift"], N, V, 32,
                                           R.EPS, None) == 2
    assert R.workspace_bytes(N, V, 32) == lib.mvd_instnorm_workspace_bytes(N, V, 32)


def test_tile_sums_and_reference_statistics_agree_with_the_two_pass_oracle():
    """the synthetic tiles are a partition: statistics from the rounded tile sums equal the two-pass fp64 ones to fp32 rounding"""
    c = next(c for c in R.CASES if c.entry == "tiles" and c.ntiles == 37 and c.xt == "fp32")
    d = R.case_data(c)
    assert d.tiles.shape == (c.N, 37, c.C, 2) and max(R.tile_sizes(c.V, 37)) <= 128
    m2 = d.x64.mean(1)
    r2 = 1.0 / (d.x64.var(1, unbiased=False) + R.EPS).sqrt()
    assert float(((d.mean - m2).abs() / d.x64.std(1)).max()) < 1e-6 and float((d.rstd / r2 - 1).abs().max()) < 1e-6
    assert float((d.x64.mean(1).abs() / d.x64.std(1)).max()) <= 2.0     # the domain of the 1-ulp bar
