"""What env sampling (rt_scene_set_env_sampling) buys and costs on one GPU, under the sun image of
tests/test_env_sampling_gpu.py (64 x 32, all (1, 1, 1) but a 4 x 4 block of 255, scale 20).  Two scenes: `shadow` -- a large Lambertian
floor with one sphere on it, no object lights -- and a scene file (default scene_500.json).  Variants: integrator 0, integrator 1 with env
sampling, and integrator 1 without it where the scene has object lights.  After one warm-up render of each they are rendered in rotation,
--repeats times; one JSON line per variant gives the median and spread of Msamples/s (host clock around rt_render) and the RMSE against a
--ref-spp integrator-0 frame of another seed, at equal samples and -- integrator 0 given the samples it traces in the time integrator 1
with env sampling needs for --spp -- at equal wall time; the last line says which side wins at equal time.
  python tools/env_sampling_run.py [--scene shadow|FILE.json] [--width W] [--height H] [--spp N] [--ref-spp N] [--repeats R]
  python tools/env_sampling_run.py --build-only     uploads the shadow scene with a 256 x 128, a 1024 x 512 and a 4096 x 2048 table (for a
                                                    `rocprofv3 --kernel-trace --stats` run of its own: the env_*_kernel rows are the build)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-raytracer_amd"))
import rtamd  # noqa: E402


def sun_image():
    img = np.ones((32, 64, 3), dtype=np.uint8)
    img[6:10, 30:34] = 255
    return img


class Deferred(rtamd.World):  # new() leaves the scene uncommitted, so that the background and the switch can still be set
    def commit(self):
        return self


def build(scene, env, size=(0, 0)):
    if scene == "shadow":
        w = Deferred()
        floor = w.XZRectangle((-1000.0, -1000.0), (1000.0, 1000.0), 0.0, w.Lambertian(w.ConstantTexture((0.6, 0.5, 0.4))))
        ball = w.Sphere((0.0, 1.0, 0.0), 1.0, w.Lambertian(w.ConstantTexture((0.7, 0.3, 0.2))))
        w.new([floor, ball], bvh_seed=1)
        cam = rtamd.Camera(((0.0, 6.0, 8.0), (0.0, 0.5, 0.0)), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0)
    else:
        w, cam = rtamd.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", scene), commit=False)
    w.set_background(texture=w.ImageTexture(sun_image()), scale=20.0)
    if env:
        w.set_env_sampling(True, *size)
    rtamd.World.commit(w)
    return w, cam


def rmse(a, b):
    return float(np.sqrt(((a - b) ** 2).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="shadow")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    if rtamd.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    if args.build_only:
        for size in ((256, 128), (1024, 512), (4096, 2048)):
            w, _ = build("shadow", True, size)
            tw, th = C.c_int(), C.c_int()
            t0 = time.perf_counter()
            rtamd._chk(w.L.rt_debug_env_table_device(w.h, 0, C.byref(tw), C.byref(th), None))  # uploads the scene: the build
            print(json.dumps({"table": "%dx%d" % (tw.value, th.value), "upload_and_build_ms_host": (time.perf_counter() - t0) * 1e3}), flush=True)
        return
    plain, cam = build(args.scene, False)
    env, _ = build(args.scene, True)
    try:  # integrator 1 without env sampling needs object lights: neither the shadow scene nor the reference's scene files have any
        plain.render(cam, width=8, height=8, spp=1, integrator=1)
        has_lights = True
    except rtamd.RtError:
        has_lights = False
    variants = [("integrator0", plain, 0), ("integrator1_env", env, 1)] + ([("integrator1", plain, 1)] if has_lights else [])
    kw = dict(width=args.width, height=args.height, seed=1)
    ref, _ = plain.render(cam, spp=args.ref_spp, integrator=0, width=args.width, height=args.height, seed=2)
    frames = {}
    for name, w, integ in variants:  # warm-up: code objects, scene upload (and table build), workspaces
        frames[name], _ = w.render(cam, spp=args.spp, integrator=integ, **kw)
    rate = {n: [] for n, _, _ in variants}
    used = {}
    for _ in range(args.repeats):
        for name, w, integ in variants:
            _, st = w.render(cam, spp=args.spp, integrator=integ, **kw)
            rate[name].append(st["samples"] / st["seconds"] / 1e6)
            used[name] = st["kernel_used"]
    med = {n: float(np.median(rate[n])) for n in rate}
    # equal wall time: integrator 0 gets the samples it traces while integrator 1 with env sampling traces --spp
    spp0 = max(1, int(round(args.spp * med["integrator0"] / med["integrator1_env"])))
    f0_time, _ = plain.render(cam, spp=spp0, integrator=0, **kw)
    for name, _, _ in variants:
        r = np.array(rate[name])
        print(json.dumps({"scene": args.scene, "size": "%dx%d" % (args.width, args.height), "spp": args.spp, "variant": name,
                          "kernel_used": used[name], "msamples_per_s_median": med[name], "msamples_per_s_min": float(r.min()),
                          "msamples_per_s_max": float(r.max()), "rmse_equal_samples": rmse(frames[name], ref), "ref_spp": args.ref_spp}), flush=True)
    e0, e1 = rmse(f0_time, ref), rmse(frames["integrator1_env"], ref)
    print(json.dumps({"scene": args.scene, "equal_time": {"integrator0_spp": spp0, "integrator0_rmse": e0, "integrator1_env_spp": args.spp,
                                                          "integrator1_env_rmse": e1},
                      "winner_at_equal_time": "integrator1_env" if e1 < e0 else "integrator0"}), flush=True)


if __name__ == "__main__":
    main()
