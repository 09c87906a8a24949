"""Tile-adaptive sampling (rt_render_adaptive) without a device: the symbols are declared and exported, the defaults are the
header's, and every bad config or partition is an argument error checked before the device."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from conftest import scene_path
from test_abi_symbols import HEADER, declared_symbols


def test_header_declares_and_library_exports_the_adaptive_entry_points():
    import rtamd
    for sym in ("rt_render_adaptive", "rt_default_adaptive_config"):
        assert sym in declared_symbols()
        assert sym in rtamd.ABI_SYMBOLS
        assert hasattr(C.CDLL(rtamd.LIB_PATH), sym)
    header = open(HEADER).read()
    assert re.search(r"typedef struct rt_adaptive_config \{\s*int32_t min_spp;.*?int32_t reserved;\s*double threshold;.*?\} rt_adaptive_config;",
                     header, flags=re.S)
    assert C.sizeof(rtamd.rt_adaptive_config) == 16


def test_default_adaptive_config_is_what_the_header_says():
    import rtamd
    c = rtamd.rt_adaptive_config(min_spp=-5, reserved=7, threshold=-1.0)
    rtamd.lib().rt_default_adaptive_config(C.byref(c))
    header = open(HEADER).read()
    body = re.search(r"typedef struct rt_adaptive_config \{(.*?)\} rt_adaptive_config;", header, flags=re.S).group(1)
    assert c.min_spp == int(re.search(r"min_spp;.*?default (\d+)", body, flags=re.S).group(1)) == 16
    assert c.threshold == float(re.search(r"threshold;.*?default ([0-9.eE+-]+)", body, flags=re.S).group(1).rstrip("."))
    assert c.threshold > 0.0 and c.reserved == 0


def _call(width=16, height=16, spp=8, min_spp=4, threshold=0.01, **params):
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    p = rtamd.default_params(width=width, height=height, spp=spp, **params)
    cfg = rtamd.rt_adaptive_config(min_spp=min_spp, reserved=0, threshold=threshold)
    out = np.zeros((height, width, 3))
    tile_spp = np.zeros(((height + 7) // 8, (width + 7) // 8), dtype=np.int32)
    rc = world.L.rt_render_adaptive(world.h, C.byref(cam.c), C.byref(p), C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_double)),
                                    tile_spp.ctypes.data_as(C.POINTER(C.c_int32)), None)
    return rc, world.L.rt_last_error()


@pytest.mark.parametrize("kw", [
    dict(min_spp=3),                     # odd
    dict(min_spp=0),                     # below 2
    dict(min_spp=-2),
    dict(min_spp=10, spp=8),             # above spp
    dict(threshold=-1e-9),               # negative
    dict(threshold=math.nan),            # NaN
    dict(world=2, rank=0),               # a tile partition
    dict(world=2, rank=1),
])
def test_bad_config_or_partition_is_an_argument_error_without_a_device(kw):
    rc, msg = _call(**kw)
    assert rc == -1, msg   # RT_ERR_ARG, before any device check


def test_a_valid_call_without_a_device_is_no_device():
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is present")
    rc, msg = _call()
    assert rc == -9, msg   # RT_ERR_NO_DEVICE: no CPU fallback
    rc, msg = _call(min_spp=8, spp=8, threshold=0.0)   # min_spp == spp and threshold 0 are valid
    assert rc == -9, msg
