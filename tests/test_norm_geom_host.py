"""The shared geometry of the row-mapped normalisation kernels (csrc/norm_common.h: norm_geom, norm_apply_chunk; no GPU): a
stand-alone host program prints both over a sweep of channel counts, batch sizes and voxel counts; the values are compared
with the Python restatement (tests/instnorm_ref.py) and with the block counts the library reports, and the bounds every
launch relies on are checked: whole waves of at most 1024 threads that hold every (channel group, row), chunks that cover
the volume, and no empty trailing block in BatchNorm's trimmed count."""
import os
import shutil
import subprocess

import pytest

import instnorm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
CS = (1, 3, 4, 5, 32, 255, 256, 320, 1023, 1024)
NS = (1, 2, 3, 2048, 4096)
VS = (1, 7, 511, 512, 4096, 8448, 2097152)


def apply_chunk(V, R_, cap):
    """about 8 rows per thread on at most `cap` blocks per sample (the rule of instnorm_ref.plan's rows())"""
    return R.cdiv(V, min(max(V // (R_ * 8), 1), max(cap, 1)))


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("norm_geom") / "norm_geom")
    cc = subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Werror",
                         "-I", os.path.join(ROOT, "multimodal_mvd_seg_amd", "csrc"),
                         os.path.join(ROOT, "tests", "host", "norm_geom_main.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return [tuple(int(w) for w in line.split()) for line in out.stdout.splitlines()]


def test_sweep_is_the_one_the_program_prints(rows):
    assert [r[:3] for r in rows] == [(C, N, V) for C in CS for N in NS for V in VS]


def test_geometry_equals_the_restatement(rows):
    for C, N, V, vec, CG, R_, threads, nblk, chunk, ach_n, ach_rb in rows:
        assert vec == (4 if C % 4 == 0 else 1) and CG * vec == C, (C, N, V)
        assert (CG, R_, threads, nblk, chunk) == R.norm_geom(N, V, C), (C, N, V)
        assert ach_n == apply_chunk(V, R_, 8192 // N), (C, N, V)
        assert ach_rb == apply_chunk(V, R_, 65535), (C, N, V)
        if vec == 4:    # the whole plan of the three-launch forward, as the InstanceNorm path tests restate it
            p = R.plan(0, N, V, C, False, False, small_max=0)
            assert (p.agrid, p.achunk) == (R.cdiv(V, ach_n), ach_n), (C, N, V)


def test_bounds_every_launch_relies_on(rows):
    for C, N, V, vec, CG, R_, threads, nblk, chunk, ach_n, ach_rb in rows:
        assert threads <= 1024 and threads % 64 == 0 and R_ * CG <= threads, (C, N, V)
        assert 1 <= nblk <= max(2048 // N, 1) and nblk * chunk >= V, (C, N, V)
        for ach, cap in ((ach_n, max(8192 // N, 1)), (ach_rb, 65535)):
            assert ach >= 1 and R.cdiv(V, ach) <= cap, (C, N, V)
        trimmed = R.cdiv(V, chunk)      # BatchNorm's count: one line after norm_geom in csrc/batchnorm.hip
        assert 1 <= trimmed <= nblk and (trimmed - 1) * chunk < V <= trimmed * chunk, (C, N, V)


def test_library_reports_these_block_counts(rows):
    from multimodal_mvd_seg_amd._lib import query
    for C, N, V, vec, CG, R_, threads, nblk, chunk, ach_n, ach_rb in rows:
        assert query("mvd_instnorm_nblk", N, V, C) == nblk, (C, N, V)
        assert query("mvd_batchnorm_nblk", N, V, C) == R.cdiv(V, chunk), (C, N, V)
