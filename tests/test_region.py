"""Pixel regions of a frame (rt_region_*), the part that needs no device: the lowering of regions to the launch's tile
list, the layout of the packed output, the order and the messages of the argument checks, and the agreement of header, Python binding,
library and Rust binding on the four symbols."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, scene_path
from region_cases import case_regions, python_tiles, small_regions

NAMES = ["rt_region_doubles", "rt_region_tiles", "rt_region_render", "rt_region_render_device"]
ARG, NOT_COMMITTED, NO_DEVICE, UNSUPPORTED = -1, -8, -9, -10


def _arr(regions):
    import rtamd
    return (rtamd.rt_region * max(1, len(regions)))(*[rtamd.rt_region(*r) for r in regions])


def _tiles(W, H, regions, capacity=None):
    """rt_region_tiles through ctypes: (return value, the ids written)"""
    import rtamd
    L = rtamd.lib()
    p = rtamd.default_params(width=W, height=H)
    n = L.rt_region_tiles(C.byref(p), len(regions), _arr(regions), 0, None)
    assert n >= 0, L.rt_last_error()
    cap = n if capacity is None else capacity
    out = np.full(max(1, n) + 4, -7, dtype=np.int32)
    ret = L.rt_region_tiles(C.byref(p), len(regions), _arr(regions), cap, out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert ret == n and (out[min(cap, n):] == -7).all()    # writes min(capacity, N) ids and nothing behind them
    return ret, out[:min(cap, n)].tolist()


# ---- rt_region_tiles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(61, 37), (64, 36)])
def test_tiles_match_the_python_restatement(W, H):
    import rtamd
    for regions in (case_regions(W, H), small_regions(W, H), small_regions(W, H)[2:5], [(W - 1, 0, W, 1)], [(0, H - 1, 1, H)]):
        n, ids = _tiles(W, H, regions)
        want = python_tiles(W, H, regions)
        assert n == len(want) and ids == want
        assert rtamd.region_tiles(W, H, regions).tolist() == want
    assert len(python_tiles(W, H, small_regions(W, H))) < ((W + 7) // 8) * ((H + 7) // 8)   # the small call leaves tiles untouched


@pytest.mark.parametrize("W,H", [(61, 37), (64, 36)])
def test_whole_frame_single_pixel_and_unaligned_window(W, H):
    total = ((W + 7) // 8) * ((H + 7) // 8)
    assert _tiles(W, H, [(0, 0, W, H)]) == (total, list(range(total)))
    assert _tiles(W, H, [(0, 0, 1, 1)]) == (1, [0])
    assert _tiles(W, H, [(W - 1, H - 1, W, H)]) == (1, [total - 1])
    tx = (W + 7) // 8
    assert _tiles(W, H, [(5, 3, 13, 11)]) == (4, [0, 1, tx, tx + 1])
    assert _tiles(W, H, [(8, 8, 16, 16)]) == (1, [tx + 1])           # an aligned 8 x 8 window is one tile


def test_the_list_is_a_function_of_the_set_of_pixels():
    W, H = 61, 37
    regions = small_regions(W, H)
    want = _tiles(W, H, regions)
    rng = np.random.default_rng(11)
    for _ in range(4):
        perm = [regions[i] for i in rng.permutation(len(regions))]
        assert _tiles(W, H, perm) == want
    assert _tiles(W, H, regions + regions[::-1] + regions[:3]) == want                       # repeated
    assert _tiles(W, H, regions + [(11, 11, 29, 24), (0, 0, 1, 1), (12, 7, 40, 8)]) == want  # regions inside the others
    # one window cut in four pieces is the same set of pixels
    assert _tiles(W, H, [(3, 2, 30, 21)]) == _tiles(W, H, [(3, 2, 17, 9), (17, 2, 30, 9), (3, 9, 17, 21), (17, 9, 30, 21)])


def test_capacity_truncates_the_writes_not_the_count():
    W, H = 61, 37
    regions = small_regions(W, H)
    want = python_tiles(W, H, regions)
    for cap in (0, 1, 5, len(want) - 1, len(want), len(want) + 3):
        n, ids = _tiles(W, H, regions, capacity=cap)
        assert n == len(want) and ids == want[:cap]


# ---- rt_region_doubles ----------------------------------------------------------------------------------------------------------------
def test_doubles_total_and_offsets():
    import rtamd
    L = rtamd.lib()
    W, H = 61, 37
    regions = case_regions(W, H)
    p = rtamd.default_params(width=W, height=H)
    sizes = [3 * (x1 - x0) * (y1 - y0) for (x0, y0, x1, y1) in regions]
    assert L.rt_region_doubles(C.byref(p), len(regions), _arr(regions)) == sum(sizes) == rtamd.region_doubles(p, regions)
    for i in range(1, len(regions) + 1):      # region i starts where regions 0 .. i-1 end
        assert L.rt_region_doubles(C.byref(p), i, _arr(regions)) == sum(sizes[:i])
    assert L.rt_region_doubles(C.byref(p), 1, _arr([(0, 0, W, H)])) == 3 * W * H


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def _call(name, world, cam, p, regions, n=None, out=True, null=()):
    """one of the four entry points with valid arguments except those named in `null`; returns (status, message)"""
    import rtamd
    L = rtamd.lib()
    n = len(regions) if n is None else n
    arr = None if "regions" in null else _arr(regions)
    pp = None if "p" in null else C.byref(p)
    buf = np.zeros(1 << 16)
    tiles = np.zeros(1 << 12, dtype=np.int32)
    if name == "rt_region_doubles":
        rc = L.rt_region_doubles(pp, n, arr)
    elif name == "rt_region_tiles":
        rc = L.rt_region_tiles(pp, n, arr, tiles.size, None if "out" in null else tiles.ctypes.data_as(C.POINTER(C.c_int32)))
    else:
        s = None if "s" in null else world.h
        c = None if "cam" in null else C.byref(cam.c)
        st = rtamd.rt_stats()
        if name == "rt_region_render":
            rc = L.rt_region_render(s, c, pp, n, arr, None if "out" in null else buf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        else:   # (a host address stands in for device memory: every case here is answered before the device is touched)
            rc = L.rt_region_render_device(s, c, pp, n, arr, None if "out" in null else C.c_void_p(buf.ctypes.data), None, C.byref(st))
    return int(rc), L.rt_last_error().decode()


@pytest.fixture(scope="module")
def scene():
    import rtamd
    return rtamd.load_scene_file(scene_path("scene_10.json"))


def _p(**kw):
    import rtamd
    args = dict(width=61, height=37, spp=4)
    args.update(kw)
    return rtamd.default_params(**args)


ONE = [(5, 3, 13, 11)]
BAD_REGIONS = {
    "empty (x0 == x1)": (7, 3, 7, 11),
    "empty (y0 == y1)": (5, 3, 13, 3),
    "reversed": (13, 3, 5, 11),
    "one pixel past the right edge": (50, 0, 62, 8),
    "one pixel past the bottom edge": (0, 30, 8, 38),
    "negative x0": (-1, 0, 8, 8),
    "negative y0": (0, -1, 8, 8),
}


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_are_rt_err_arg_with_a_message_that_names_the_defect(name, scene):
    world, cam = scene
    nulls = ["p", "regions"] + (["s", "cam", "out"] if "render" in name else [])
    for which in nulls:
        assert _call(name, world, cam, _p(), ONE, null=(which,)) == (ARG, "null argument"), which
    if name == "rt_region_tiles":
        rc, msg = _call(name, world, cam, _p(), ONE, null=("out",))
        assert rc == ARG and "out_tiles" in msg and "capacity" in msg
    # anything make_plan refuses
    for kw, word in [(dict(width=0), "width/height"), (dict(height=-3), "width/height"), (dict(spp=0), "spp"), (dict(max_depth=-1), "max_depth"),
                     (dict(kernel=4), "kernel"), (dict(integrator=3), "integrator"), (dict(time0=1.0, time1=0.5), "shutter")]:
        rc, msg = _call(name, world, cam, _p(**kw), ONE)
        assert rc == ARG and word in msg, (kw, msg)
    for kw in (dict(world=2), dict(world=2, rank=1)):
        rc, msg = _call(name, world, cam, _p(**kw), ONE)
        assert rc == ARG and "world must be 1" in msg, (kw, msg)
    rc, msg = _call(name, world, cam, _p(world=1, rank=1), ONE)
    assert rc == ARG and "rank" in msg
    for n in (0, -1, 65537):
        rc, msg = _call(name, world, cam, _p(), ONE * 2, n=n)
        assert rc == ARG and "n_regions must be 1..65536" in msg, (n, msg)
    for what, bad in BAD_REGIONS.items():
        rc, msg = _call(name, world, cam, _p(), [ONE[0], bad, ONE[0]])
        assert rc == ARG, what
        assert "region 1 = (%d, %d, %d, %d)" % bad in msg and "width = 61" in msg and "height = 37" in msg, (what, msg)
    # the frame's own edge is inside
    assert _call("rt_region_doubles", world, cam, _p(), [(60, 36, 61, 37), (0, 0, 61, 37)])[0] == 3 * (1 + 61 * 37)


def test_65536_regions_are_accepted():
    import rtamd
    p = _p()
    regions = [(i % 61, i % 37, i % 61 + 1, i % 37 + 1) for i in range(65536)]
    assert rtamd.region_doubles(p, regions) == 3 * 65536
    assert rtamd.region_tiles(61, 37, regions).tolist() == python_tiles(61, 37, regions[:61 * 37])


@pytest.mark.parametrize("name", NAMES[2:])
def test_statuses_in_the_order_of_the_header(name, scene):
    """RT_ERR_ARG, then RT_ERR_UNSUPPORTED (kernel 6, integrator 2), then RT_ERR_NOT_COMMITTED (RT_ERR_NO_DEVICE comes last: below)"""
    import rtamd
    world, cam = scene
    fresh = rtamd.World()                                           # never committed
    for kw in (dict(kernel=6), dict(integrator=2)):
        for w in (world, fresh):
            rc, msg = _call(name, w, cam, _p(**kw), ONE)
            assert rc == UNSUPPORTED and "kernels 0 / 1 / 2 / 5 and integrators 0 / 1" in msg, (kw, msg)
        assert _call(name, fresh, cam, _p(**kw), [(0, 0, 62, 8)])[0] == ARG      # an argument error comes first
    assert _call(name, fresh, cam, _p(), ONE)[0] == NOT_COMMITTED
    assert _call(name, fresh, cam, _p(), [(0, 0, 62, 8)])[0] == ARG


@pytest.mark.parametrize("name", NAMES[2:])
def test_a_valid_call_without_a_device_is_rt_err_no_device(name, scene):
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is present")
    world, cam = scene
    rc, msg = _call(name, world, cam, _p(), case_regions(61, 37))
    assert rc == NO_DEVICE and "no HIP device" in msg


def test_python_wrappers_raise_rt_error(scene):
    import rtamd
    world, cam = scene
    with pytest.raises(rtamd.RtError) as e:
        world.render_region(cam, (0, 0, 62, 8), width=61, height=37, spp=2)
    assert e.value.code == ARG and "region 0 = (0, 0, 62, 8)" in str(e.value)
    with pytest.raises(rtamd.RtError) as e:
        world.render_regions(cam, [], width=61, height=37, spp=2)
    assert e.value.code == ARG and "n_regions" in str(e.value)
    with pytest.raises(rtamd.RtError) as e:
        rtamd.region_tiles(61, 37, [(0, 0, 8, 38)])
    assert e.value.code == ARG
    if rtamd.device_count() < 1:
        with pytest.raises(rtamd.RtError) as e:
            world.render_region(cam, (0, 0, 8, 8), width=61, height=37, spp=2)
        assert e.value.code == NO_DEVICE


# ---- the four symbols, everywhere -------------------------------------------------------------------------------------------------------
def test_header_binding_library_and_rust_agree_on_the_region_symbols():
    import rtamd
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtamd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_region_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NAMES)
    assert sorted(s for s in rtamd.ABI_SYMBOLS if s.startswith("rt_region")) == declared
    L = C.CDLL(rtamd.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), "librtamd.so does not export %s" % name
    rs = open(os.path.join(ROOT, "rust-raytracer_amd", "rust", "rtamd_ffi.rs")).read()
    ext = rs[rs.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    rust = dict((m.group(1), m.group(2)) for m in re.finditer(r"pub fn (rt_region_[a-z0-9_]+)\((.*?)\)", ext, flags=re.S))
    assert sorted(rust) == declared
    for name, args in rust.items():
        c_args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, header, flags=re.S).group(1).split(",")
        assert len(c_args) == len(args.split(",")), name
    assert re.search(r"#\[repr\(C\)\]\n(?:#\[derive\([^)]*\)\]\n)?pub struct rt_region \{\s*pub x0: i32,\s*pub y0: i32,\s*pub x1: i32,\s*pub y1: i32,\s*\}", rs)
    assert "pub fn render_regions(" in rs
    assert C.sizeof(rtamd.rt_region) == 16 and [f for f, _ in rtamd.rt_region._fields_] == ["x0", "y0", "x1", "y1"]
    assert re.search(r"typedef struct rt_region \{ int32_t x0, y0, x1, y1; \} rt_region;", header)
    assert rtamd.lib().rt_abi_version() == 2        # no struct changed


def test_no_new_symbol_looks_like_a_render_entry_point():
    """tests/test_render_entry_errors.py wants every header symbol rt_(render|accum)* in its recorded table: the region entry points keep
    out of that pattern, and the header's set of such symbols is still the table's"""
    header = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    table = json.load(open(os.path.join(GOLDEN, "render_entry_table.json")))
    declared = set(re.findall(r"\b(rt_(?:render|accum)\w*)\s*\(", header))
    assert declared <= set(table["entries"]), sorted(declared - set(table["entries"]))
    for name in NAMES:
        assert not re.match(r"rt_(render|accum)\w*", name) and name not in table["entries"]
