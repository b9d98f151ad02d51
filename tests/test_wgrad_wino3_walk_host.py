"""The scalar tile walk of k_wgrad_wino3 (csrc/conv_geom.h: tile_walk_at / tile_walk_advance, no GPU): a stand-alone host
program walks every split of every split count over small tile grids (extents of 1 included) and a few strided walks
over grids at the entry point's limit of 2^30 tiles, and compares each visited tile with plain division.  The walk has
no product limit of its own (it never multiplies): a digit plus a digit plus a carry is below twice the extent, which
the small grids exercise at every carry pattern, and the large grids cover the magnitudes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
def test_walk_equals_division(tmp_path):
    exe = str(tmp_path / "wgrad_walk")
    cc = subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Werror",
                         "-I", os.path.join(ROOT, "multimodal_mvd_seg_amd", "csrc"),
                         os.path.join(ROOT, "tests", "host", "wgrad_walk_main.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10 ** 6
