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


def _route_from_queries(N, sp, C1, C2, K, ks, st):
    """The engine of each pass as Conv3dFn combined it from the three queries before mvd_conv3d_route existed: the 3-D bits
    win over the F(2x2,3x3) bits, the in-plane engine for (1,3,3), direct otherwise"""
    wino = _bits("mvd_conv_wino_applicable", N, sp, C1, C2, K, ks, st)
    wino3 = _bits("mvd_conv_wino3_applicable", N, sp, C1, C2, K, ks, st) if wino else 0
    wino2 = wino & ~wino3
    wino2p = _bits("mvd_conv_wino2p_applicable", N, sp, C1, C2, K, ks, st) if tuple(ks) == (1, 3, 3) else 0
    assert not (wino2p and wino), "a pass cannot have a 27-tap and a 9-tap engine"
    kind = lambda bit: (_lib.CONV_WINO3 if wino3 & bit else _lib.CONV_WINO2 if wino2 & bit else
                        _lib.CONV_WINO2P if wino2p & bit else _lib.CONV_DIRECT)
    return kind(1) | (kind(2) << 4)


@pytest.mark.parametrize("mins", [(-1, -1, -1), (1, 1, 1), (1, 3, 1)], ids=["defaults", "all-1", "raised-3d"])
def test_route_is_the_combination_of_the_three_queries(mins):
    """mvd_conv3d_route over batch, extent, channels (with non-multiples of 32), the four kernel sizes and the three strides,
    under default minimums, under all minimums 1 and under a raised 3-D minimum (3 items per sample: 8^3 x 64 channels has
    2 x 2 = 4, 4x8x8 x 64 has 2, so forward and input gradient differ where K != C1 + C2)"""
    _lib.load()
    if _lib.query("mvd_wino_mode") == 0:
        pytest.skip("MVD_WINO=0 for this run")
    setters = ("mvd_set_wino_min_items", "mvd_set_wino3_min_items", "mvd_set_wino2p_min_items")
    seen = set()
    try:
        for fn, n in zip(setters, mins):
            _lib.call(fn, n)
        for N in (1, 2):
            for sp in ((1, 40, 48), (4, 8, 8), (5, 6, 7), (8, 8, 8), (32, 32, 32), (128, 128, 128)):
                for C1, C2, K in ((32, 0, 32), (32, 0, 96), (96, 0, 32), (32, 32, 64), (64, 32, 32), (4, 0, 32), (32, 0, 33),
                                  (32, 16, 32), (256, 0, 256)):
                    for ks in ((3, 3, 3), (1, 3, 3), (3, 3, 1), (1, 1, 1)):
                        for st in ((1, 1, 1), (2, 2, 2), (1, 2, 2)):
                            got = _bits("mvd_conv3d_route", N, sp, C1, C2, K, ks, st)
                            assert got == _route_from_queries(N, sp, C1, C2, K, ks, st), (N, sp, C1, C2, K, ks, st)
                            seen.add(got)
    finally:
        for fn in setters:
            _lib.call(fn, -1)
    # the grid reaches every engine in both passes (with every minimum at 1 the 3-D engine takes all that F(2x2,3x3) would),
    # and mixed routes
    assert {k & 15 for k in seen} == {k >> 4 for k in seen} == ({0, 2, 3} if mins == (1, 1, 1) else {0, 1, 2, 3})
    if mins == (1, 3, 1):
        assert any((k & 15) != (k >> 4) for k in seen)


def test_wino3_env_switch_turns_the_engine_off():
    code = ("from multimodal_mvd_seg_amd import _lib; _lib.load(); "
            "print(_lib.query('mvd_conv_wino3_applicable', 2, 128, 128, 128, 32, 0, 32, _lib.i3((3, 3, 3)), _lib.i3((1, 1, 1))), "
            "_lib.query('mvd_conv_wino_applicable', 2, 128, 128, 128, 32, 0, 32, _lib.i3((3, 3, 3)), _lib.i3((1, 1, 1))))")
    env = dict(os.environ, MVD_WINO3="0", PYTHONPATH=ROOT)
    env.pop("MVD_WINO", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "3"]
