"""Nested Transforms on the host (no GPU): scenes whose Transforms nest up to the documented maximum (8 levels) commit with an accel
(one object-space BVH per chain of Transforms), deeper ones
and lights under a Transform are refused with RT_ERR_UNSUPPORTED, bounding boxes of nested Transforms agree with the oracle bit for
bit, and the flattened scene of every existing configuration -- depth <= 1 -- is byte-identical to what it was before nesting was
supported (fingerprints and rt_scene_info recorded on the build before the change: tests/golden/nested_transform_pins.json)."""
import glob
import json
import os
import sys

import numpy as np
import pytest

import nested_scenes as ns
from conftest import GOLDEN, ROOT, SCENES

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402


def _world():
    import rtamd
    return rtamd.World()


@pytest.mark.parametrize("levels", [2, 3, ns.MAX_DEPTH])
def test_nested_chains_commit(levels):
    w, _ = ns.n7(_world(), levels=levels)
    info = w.info()
    assert info["committed"] == 1 and info["n_xforms"] == levels
    # one object-space BVH per chain level (the Transforms of n7 are not shared), one REF_RESTORE entry per level on the stack
    assert info["accel_ok"] == 1 and info["accel_instances"] == levels and info["accel_compact"] == 0
    assert info["accel_stack"] >= levels + 2


@pytest.mark.parametrize("name", sorted(ns.SCENES))
def test_gpu_scenes_commit(name):
    w, _ = ns.SCENES[name](_world())
    info = w.info()
    # n6: a ConstantMedium under a Transform is kernel 1's only, at any depth
    assert info["committed"] == 1 and info["accel_ok"] == (0 if name == "n6" else 1) and info["accel_compact"] == 0


def test_deeper_than_the_limit_is_refused():
    import rtamd
    with pytest.raises(rtamd.RtError) as e:
        ns.n7(_world(), levels=ns.MAX_DEPTH + 1)
    assert e.value.code == -10 and "8 levels" in str(e.value)


def test_light_under_a_nested_transform_is_refused():
    import rtamd
    w = _world()
    white, items = ns.walls(w)
    lt = ns.light(w)
    t = ns.nest(w, [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, -1.0, 0.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))], lt)
    with pytest.raises(rtamd.RtError) as e:
        w.new(items + [t], lights=[lt])
    assert e.value.code == -10


def test_shared_inner_transform_gets_one_context_per_chain():
    """n3: the inner Transform under two outer ones and at world level is three chains, each with its own object-space BVH"""
    w, _ = ns.n3(_world())
    # chains: o1, o2, o1/inner, o1/ball, o2/inner, o2/ball, inner, ball
    assert w.info()["accel_instances"] == 8 and w.info()["n_xforms"] == 4


def test_depth_one_scene_is_unchanged_by_a_shared_transform():
    """a Transform used twice at depth 1 is one chain: the scene stays a depth-1 scene (accel built)"""
    w = _world()
    white, items = ns.walls(w)
    t = w.Transform((0.0, 30.0, 0.0), (1.0, 1.0, 1.0), (100.0, 0.0, 100.0), w.Cube((0.0, 0.0, 0.0), (50.0, 50.0, 50.0), white))
    w.new(items + [t, t], bvh_seed=1)
    assert w.info()["accel_ok"] == 1


def test_bounding_boxes_of_nested_transforms_match_the_oracle():
    import oracle
    w, o = _world(), oracle.Scene()
    objs = []
    for B in (w, o):
        m = B.Lambertian(B.ConstantTexture((0.5, 0.5, 0.5)))
        prims = [B.Sphere((1.0, 2.0, 3.0), 0.5, m), B.Cube((0.0, -1.0, 2.0), (1.0, 2.0, 3.5), m), B.XZRectangle((0.0, 1.0), (2.0, 3.0), 4.0, m)]
        out = []
        for k, p in enumerate(prims):
            for levels in (2, 3, 5, ns.MAX_DEPTH):
                out.append(ns.nest(B, ns.chain(levels)[k:] + ns.chain(levels)[:k], p))
        inner = ns.nest(B, ns.chain(2), prims[1])
        out.append(B.Transform((10.0, 20.0, 30.0), (2.0, 0.5, 3.0), (4.0, 5.0, 6.0), ns.bvh(B, [inner, prims[0], ns.nest(B, ns.chain(3), prims[2])], 3)))
        out.append(B.Transform((-45.0, 0.0, 60.0), (0.25, 4.0, 1.0), (0.0, 0.0, 0.0), B.Transform((0.0, 90.0, 0.0), (1.0, 1.0, 7.0), (1.0, 1.0, 1.0), inner)))
        objs.append(out)
    for a, b in zip(*objs):
        assert np.array_equal(w.bounding_box(a), o.bounding_box(b))


def _pin_keys():
    return list(configs.CONFIGS) + [os.path.basename(p) for p in sorted(glob.glob(os.path.join(SCENES, "scene_*.json")))]


@pytest.mark.parametrize("key", _pin_keys())
def test_depth_le_1_blobs_are_unchanged(key):
    import rtamd
    pins = json.load(open(os.path.join(GOLDEN, "nested_transform_pins.json")))
    w, _ = configs.product(key) if key in configs.CONFIGS else rtamd.load_scene_file(os.path.join(SCENES, key))
    assert "%016x" % w.L.rt_scene_fingerprint(w.h) == pins[key]["fingerprint"]
    assert w.info() == pins[key]["info"]
