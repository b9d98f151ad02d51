"""The geometry descriptors of csrc/conv_geom.h (no GPU): tests/host/conv_geom_dump.cpp builds every descriptor the conv
entry points hand to the kernels -- forward, each input-gradient parity class, weight gradient, the transposed-conv ones --
for a fixed problem list, and its output must equal tests/golden/conv_geom.txt byte for byte.  The golden was recorded from
the builder bodies as they stood in conv.hip (one copy per precision) before conv_geom.h became their only home."""
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
def test_descriptors_match_the_recorded_bytes(tmp_path):
    exe = str(tmp_path / "conv_geom_dump")
    cc = subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Werror",
                         "-I", os.path.join(ROOT, "multimodal_mvd_seg_amd", "csrc"),
                         os.path.join(ROOT, "tests", "host", "conv_geom_dump.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    want = open(os.path.join(GOLDEN, "conv_geom.txt")).read().splitlines()
    assert len(want) > 300
    assert [l.rsplit(" ", 1)[0] for l in got] == [l.rsplit(" ", 1)[0] for l in want]  # the same descriptors, in order
    for g, w in zip(got, want):
        assert g == w, g.rsplit(" ", 1)[0]
