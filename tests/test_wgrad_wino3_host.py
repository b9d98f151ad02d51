"""Host logic of the F(2x2x2,3x3x3) weight-gradient selection (no GPU): which shapes it serves, its minimum of work
items per sample (independent of the batch size) and the MVD_WGRAD_WINO3=0 switch."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from multimodal_mvd_seg_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libmvdseg_hip.so not built")


def _on(N, sp, C1, C2, K, ks=(3, 3, 3), st=(1, 1, 1)):
    return _lib.query("mvd_conv_wgrad_wino3_applicable", N, *sp, C1, C2, K, _lib.i3(ks), _lib.i3(st))


def test_wgrad_wino3_shapes_and_minimum():
    _lib.load()
    if _lib.query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0 for this run")
    try:
        _lib.call("mvd_set_wgrad_wino3_min_items", 1)
        assert _on(1, (8, 8, 8), 32, 32, 64) == 1
        assert _on(1, (5, 7, 9), 32, 0, 32) == 1
        # only plain 3x3x3 stride-1 convs with 32-multiple channels
        assert _on(1, (8, 8, 8), 32, 0, 32, st=(2, 2, 2)) == 0
        assert _on(1, (8, 8, 8), 32, 0, 32, ks=(1, 1, 1)) == 0
        assert _on(1, (8, 8, 8), 4, 0, 32) == 0
        assert _on(1, (8, 8, 8), 32, 16, 32) == 0
        assert _on(1, (8, 8, 8), 32, 0, 48) == 0
        # items per sample = 2x8x8 tiles x (C/32) x (K/32): 4 x 1 x 1 x 2 x 2 = 16 at 8^3, 64 + 64 -> 64
        _lib.call("mvd_set_wgrad_wino3_min_items", 16)
        assert _on(1, (8, 8, 8), 32, 32, 64) == 1
        _lib.call("mvd_set_wgrad_wino3_min_items", 17)
        assert _on(1, (8, 8, 8), 32, 32, 64) == 0
        # ... counted per sample: the batch size never changes the choice
        for n in (1, 2, 3, 8):
            assert _on(n, (8, 8, 8), 32, 32, 64) == 0
        _lib.call("mvd_set_wgrad_wino3_min_items", 16)
        for n in (1, 2, 3, 8):
            assert _on(n, (8, 8, 8), 32, 32, 64) == 1
        _lib.call("mvd_set_wgrad_wino3_min_items", 1 << 40)
        assert _on(2, (128, 128, 128), 32, 32, 32) == 0
        # defaults: the same answer at batch 1 and 2 for every stride-1 fp32 layer of configs[1]
        _lib.call("mvd_set_wgrad_wino3_min_items", -1)
        for S, C1, C2, K in [(128, 32, 0, 32), (128, 32, 32, 32), (64, 64, 0, 64), (64, 64, 64, 64), (32, 128, 0, 128),
                             (32, 128, 128, 128), (16, 256, 0, 256), (16, 256, 256, 256)]:
            assert _on(1, (S, S, S), C1, C2, K) == _on(2, (S, S, S), C1, C2, K)
        assert _on(2, (128, 128, 128), 32, 32, 32) == 1
        assert _on(2, (64, 64, 64), 64, 0, 64) == 1
    finally:
        _lib.call("mvd_set_wgrad_wino3_min_items", -1)


def test_wgrad_wino3_workspace_holds_64_positions():
    _lib.load()
    # 64 positions x C x K per split (one workgroup per CU: 256 / (C/32 * K/32) splits) + two bias rows per split
    for C, K in [(32, 32), (64, 32), (64, 64), (256, 128), (512, 256)]:
        ns = max(1, 256 // ((C // 32) * (K // 32)))
        need = ns * (64 * C + 2) * K * 4
        assert _lib.query("mvd_conv3d_wgrad_workspace_bytes", C, K, 27, 2, 16, 16, 16) >= need


def test_wgrad_wino3_env_switch_turns_the_engine_off():
    code = ("from multimodal_mvd_seg_amd import _lib; _lib.load(); "
            "print(_lib.query('mvd_conv_wgrad_wino3_applicable', 2, 128, 128, 128, 32, 32, 32, _lib.i3((3, 3, 3)), "
            "_lib.i3((1, 1, 1))))")
    env = dict(os.environ, MVD_WGRAD_WINO3="0", PYTHONPATH=ROOT)
    env.pop("MVD_WINO", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0"]
