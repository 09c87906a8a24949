"""What a background (rt_scene_set_background) costs on one GPU.  The same scene file is committed three times -- without a
background, with a black one (kind 1, colour 0: the background variants, bit-identical frames) and with book 1's sky -- and rendered in
rotation (none, black, sky, none, black, sky, ...) after one warm-up render of each, so that clock drift spreads over all three.  Prints
one JSON line per variant: the median and spread of Msamples/s (host clock around rt_render, which returns after the frame is copied to
the host) and of the kernel time, the kernel that ran, and whether the black frame equals the frame without a background.
usage: python tools/background_run.py [--scene scene_500.json] [--width W] [--height H] [--spp N] [--repeats R] [--kernel K]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-raytracer_amd"))
import rtamd  # noqa: E402

VARIANTS = (("none", None), ("black", dict(color=(0.0, 0.0, 0.0))), ("sky", dict(gradient=rtamd.SKY)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="scene_500.json")
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--spp", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel", type=int, default=0)
    args = ap.parse_args()
    if rtamd.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    path = os.path.join(ROOT, "tests", "golden", "scenes", args.scene)
    worlds = {}
    for name, bg in VARIANTS:
        w, cam = rtamd.load_scene_file(path, commit=False)
        if bg is not None:
            w.set_background(**bg)
        worlds[name] = w.commit()
    kw = dict(width=args.width, height=args.height, spp=args.spp, seed=1, kernel=args.kernel)
    frames = {}
    for name, _ in VARIANTS:  # warm-up: code objects, scene upload, workspaces
        frames[name], _ = worlds[name].render(cam, **kw)
    rate = {n: [] for n, _ in VARIANTS}
    kms = {n: [] for n, _ in VARIANTS}
    used = {}
    for _ in range(args.repeats):
        for name, _ in VARIANTS:
            _, st = worlds[name].render(cam, **kw)
            rate[name].append(st["samples"] / st["seconds"] / 1e6)
            kms[name].append(st["kernel_ms"])
            used[name] = st["kernel_used"]
    for name, _ in VARIANTS:
        r = np.array(rate[name])
        print(json.dumps({"scene": args.scene, "size": "%dx%d" % (args.width, args.height), "spp": args.spp, "background": name,
                          "kernel_used": used[name], "msamples_per_s_median": float(np.median(r)), "msamples_per_s_min": float(r.min()),
                          "msamples_per_s_max": float(r.max()), "kernel_ms_median": float(np.median(kms[name])),
                          "relative_to_none": float(np.median(r) / np.median(rate["none"])),
                          "equals_none": bool(np.array_equal(frames[name], frames["none"])),
                          "pixels_brighter_than_none": float((frames[name] > frames["none"]).any(axis=-1).mean())}), flush=True)


if __name__ == "__main__":
    main()
