"""What area lights (rt_scene_set_area_lights) cost and buy on one GPU.  One JSON line per measurement:
  scene    the scene of tests/test_area_lights_gpu.py (a floor, two balls, an emissive YZ window and an emissive tetrahedron under a
           Transform): integrator 0 against integrator 1, Msamples/s and the per-pixel variance across seeds;
  cornell  the Cornell box with its lamp declared as an object light (rt_scene_set_lights) and as an area light (2 triangles), both
           under integrator 1;
  bounce   one diffuse bounce, isolated: a floor that fills the frame under a mesh light of 12, 128 and 1024 triangles at max_depth 1, so
           every sample runs the mixture step exactly once; ns per sample of integrator 1 minus integrator 0's on the same scene.
Variants are rendered in rotation after a warm-up, --repeats times; rates are medians of samples / kernel time.
  python tools/area_lights_run.py [--width W] [--height H] [--spp N] [--repeats R]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtamd  # noqa: E402


def rotate(variants, repeats, **kw):
    """[(name, world, camera, render kwargs)] -> {name: (median Msamples/s by kernel time, min, max, kernel used)}"""
    for _, w, cam, extra in variants:  # warm-up: code objects, scene upload, workspaces
        w.render(cam, **dict(kw, **extra))
    rate = {n: [] for n, _, _, _ in variants}
    used = {}
    for _ in range(repeats):
        for name, w, cam, extra in variants:
            _, st = w.render(cam, **dict(kw, **extra))
            rate[name].append(st["samples"] / (st["kernel_ms"] * 1e-3) / 1e6)
            used[name] = st["kernel_used"]
    return {n: (float(np.median(r)), float(min(r)), float(max(r)), used[n]) for n, r in rate.items()}


def report(what, res, **more):
    for name, (med, lo, hi, kernel) in res.items():
        print(json.dumps(dict(measurement=what, variant=name, kernel_used=kernel, msamples_per_s_median=med, msamples_per_s_min=lo,
                              msamples_per_s_max=hi, ns_per_sample=1e3 / med, **more)), flush=True)


def cornell(as_area):
    w, cam = rtamd.select_scene(os.path.join(ROOT, "tests", "golden", "scenes", "cube.obj"), 1.0, 1, commit=False)
    if as_area:
        lamp = []
        for o in range(w.root() + 1):  # (object ids count up; the root was made last)
            kind, d = w.describe(o)
            if kind == "Rect" and d["axis"] == 1 and d["v"][4] == 554.0:
                lamp.append(o)
        assert len(lamp) == 1
        w.set_lights([])
        w.set_area_lights(lamp)
    return w.commit(), cam


def bounce_scene(n_tri):
    """a floor that fills the frame, lit by a strip mesh of n_tri emissive triangles over a 2 x 1 rectangle 3 above it"""
    w = rtamd.World()
    floor = w.XZRectangle((-100.0, -100.0), (100.0, 100.0), 0.0, w.Lambertian(w.ConstantTexture((0.7, 0.7, 0.7))))
    cols = n_tri // 2
    pos = np.array([[-1.0 + 2.0 * (i // 2) / cols, 3.0, -0.5 + (i % 2)] for i in range(2 * cols + 2)])
    idx = [(i, i + 1, i + 2) for i in range(2 * cols)]
    light = w.Mesh(pos, np.tile([0.0, -1.0, 0.0], (len(pos), 1)), idx, w.DiffuseLight(w.ConstantTexture((10.0, 10.0, 10.0))))
    w.new([floor, light], area_lights=[light])
    assert len(w.area_light_tris()) == n_tri
    return w, rtamd.Camera(((0.0, 2.0, 0.0), (0.0, 0.0, 0.1)), (0.0, 0.0, 1.0), 40.0, 1.0, 0.0, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if rtamd.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    kw = dict(width=args.width, height=args.height, spp=args.spp, seed=1)

    import test_area_lights_gpu as t
    w, cam = t.scene(), t._camera()
    report("scene", rotate([("integrator0", w, cam, dict(integrator=0)), ("integrator1_area", w, cam, dict(integrator=1))], args.repeats, **kw))
    var = {}
    for integ in (0, 1):
        frames = np.array([w.render(cam, width=64, height=64, spp=16, seed=500 + k, integrator=integ)[0] for k in range(16)])
        var[integ] = float(frames.var(axis=0, ddof=1).mean())
    print(json.dumps(dict(measurement="scene", variance_integrator0=var[0], variance_integrator1=var[1], ratio=var[1] / var[0])), flush=True)

    wo, cam = cornell(False)
    wa, _ = cornell(True)
    report("cornell", rotate([("integrator1_object_light", wo, cam, dict(integrator=1)), ("integrator1_area_light", wa, cam, dict(integrator=1)),
                              ("integrator1_object_light_kernel2", wo, cam, dict(integrator=1, kernel=2))], args.repeats, **kw))

    for n_tri in (12, 128, 1024):
        w, cam = bounce_scene(n_tri)
        res = rotate([("integrator0", w, cam, dict(integrator=0)), ("integrator1_area", w, cam, dict(integrator=1))], args.repeats,
                     max_depth=1, **kw)
        report("bounce", res, light_triangles=n_tri)
        print(json.dumps(dict(measurement="bounce", light_triangles=n_tri,
                              mixture_step_ns_per_sample=1e3 / res["integrator1_area"][0] - 1e3 / res["integrator0"][0])), flush=True)


if __name__ == "__main__":
    main()
