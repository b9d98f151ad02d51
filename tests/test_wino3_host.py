"""Host logic of the F(2x2x2,3x3x3) engine selection (no GPU): 3-D, then F(2x2,3x3), then direct, under both minimum
item counts and MVD_WINO3=0."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from multimodal_mvd_seg_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libmvdseg_hip.so not built")


def _bits(fn, N, sp, C1, C2, K, ks=(3, 3, 3), st=(1, 1, 1)):
    return _lib.query(fn, N, *sp, C1, C2, K, _lib.i3(ks), _lib.i3(st))


def test_wino3_selection_follows_both_minimums():
    _lib.load()
    if _lib.query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0 for this run")
    try:
        _lib.call("mvd_set_wino_min_items", 1)
        _lib.call("mvd_set_wino3_min_items", 1)
        assert _bits("mvd_conv_wino3_applicable", 1, (8, 8, 8), 32, 32, 64) == 3
        # never where the F(2x2,3x3) engine does not apply: strides, 1x1x1, channels that are not multiples of 32
        assert _bits("mvd_conv_wino3_applicable", 1, (8, 8, 8), 32, 0, 32, st=(2, 2, 2)) == 0
        assert _bits("mvd_conv_wino3_applicable", 1, (8, 8, 8), 32, 0, 32, ks=(1, 1, 1)) == 0
        assert _bits("mvd_conv_wino3_applicable", 1, (8, 8, 8), 4, 0, 32) == 0
        # the 3-D minimum counts 4x8x8-voxel x 32-channel items per sample, separately for the forward (K) and the
        # dgrad (C1+C2); the batch size does not enter
        _lib.call("mvd_set_wino3_min_items", 3)
        assert _bits("mvd_conv_wino3_applicable", 4, (4, 8, 8), 64, 0, 64) == 0
        _lib.call("mvd_set_wino3_min_items", 2)
        assert _bits("mvd_conv_wino3_applicable", 1, (4, 8, 8), 32, 0, 64) == 1
        assert _bits("mvd_conv_wino3_applicable", 1, (4, 8, 8), 64, 0, 32) == 2
        assert _bits("mvd_conv_wino_applicable", 1, (4, 8, 8), 64, 0, 32) == 3
        # the F(2x2,3x3) minimum gates the 3-D engine too
        _lib.call("mvd_set_wino_min_items", 1 << 40)
        assert _bits("mvd_conv_wino3_applicable", 2, (64, 64, 64), 32, 0, 32) == 0
        _lib.call("mvd_set_wino_min_items", -1)
        _lib.call("mvd_set_wino3_min_items", -1)
        # defaults: every Winograd layer of the flagship (batch 2) down to 16^3 x 256 channels takes the 3-D engine,
        # whatever the batch; a 2-D-only layer: 16^3 x 256 (128 3-D items per sample) below a raised 3-D minimum
        assert _bits("mvd_conv_wino3_applicable", 1, (32, 32, 32), 32, 0, 32) == 3
        assert _bits("mvd_conv_wino3_applicable", 2, (32, 32, 32), 32, 0, 32) == 3
        assert _bits("mvd_conv_wino3_applicable", 2, (128, 128, 128), 32, 0, 32) == 3
        assert _bits("mvd_conv_wino3_applicable", 2, (64, 64, 64), 64, 0, 64) == 3
        assert _bits("mvd_conv_wino3_applicable", 2, (16, 16, 16), 256, 0, 256) == 3
        _lib.call("mvd_set_wino3_min_items", 129)
        assert _bits("mvd_conv_wino3_applicable", 2, (16, 16, 16), 256, 0, 256) == 0
        assert _bits("mvd_conv_wino_applicable", 2, (16, 16, 16), 256, 0, 256) == 3
        assert _lib.query("mvd_wino3_weight_elems", 32, 64) == 64 * 32 * 64
    finally:
        _lib.call("mvd_set_wino_min_items", -1)
        _lib.call("mvd_set_wino3_min_items", -1)


def test_wino3_env_switch_turns_the_engine_off():
    code = ("from multimodal_mvd_seg_amd import _lib; _lib.load(); "
            "print(_lib.query('mvd_conv_wino3_applicable', 2, 128, 128, 128, 32, 0, 32, _lib.i3((3, 3, 3)), _lib.i3((1, 1, 1))), "
            "_lib.query('mvd_conv_wino_applicable', 2, 128, 128, 128, 32, 0, 32, _lib.i3((3, 3, 3)), _lib.i3((1, 1, 1))))")
    env = dict(os.environ, MVD_WINO3="0", PYTHONPATH=ROOT)
    env.pop("MVD_WINO", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "3"]
