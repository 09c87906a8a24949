"""What a region call (rt_region_render) costs on one GPU beside the whole frame, on the headline scene: rt_render, the
whole frame as one region, one aligned 64 x 64 region and the eleven 8 x 8 windows of tests/test_golden.py.  After one warm-up call of
each the four are made in rotation, --repeats times; one JSON line per case gives the medians of the call's wall time (rt_stats.seconds)
and of its path-trace kernel time (rt_stats.kernel_ms), the tiles and the samples it traced, and checks the regions against the frame.
  python tools/region_run.py [--scene FILE.json] [--width W] [--height H] [--spp N] [--repeats R]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rust-raytracer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import rtamd  # noqa: E402
from seeded_windows import seeded_windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "scene_500.json"))
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if rtamd.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    W, H = a.width, a.height
    world, cam = rtamd.load_scene_file(a.scene)
    kw = dict(width=W, height=H, spp=a.spp, seed=1)
    x64, y64 = (W // 2) // 64 * 64, (3 * H // 4) // 64 * 64
    windows = [(x0, y0, x0 + 8, y0 + 8) for (x0, y0) in [(W // 2, 3 * H // 4), (296 * W // 1200, 640 * H // 1200), (1000 * W // 1200, 40 * H // 1200)]
               + seeded_windows(W, H, 1000)]
    cases = [("rt_render", None), ("whole-frame region", [(0, 0, W, H)]), ("one aligned 64x64 region", [(x64, y64, x64 + 64, y64 + 64)]),
             ("eleven 8x8 windows", windows)]

    def call(regions):
        if regions is None:
            img, st = world.render(cam, **kw)
            return [img], st
        return world.render_regions(cam, regions, **kw)

    frame = call(None)[0][0]
    for _, regions in cases[1:]:                                    # warm-up, and the regions are the frame's pixels
        views, _ = call(regions)
        for v, (x0, y0, x1, y1) in zip(views, regions):
            assert np.array_equal(v, frame[y0:y1, x0:x1]), (x0, y0, x1, y1)
    runs = {name: [] for name, _ in cases}
    for _ in range(a.repeats):
        for name, regions in cases:
            runs[name].append(call(regions)[1])
    for name, regions in cases:
        st = runs[name]
        sec = [s["seconds"] for s in st]
        print(json.dumps({"case": name, "tiles": int(rtamd.region_tiles(W, H, regions).size) if regions else ((W + 7) // 8) * ((H + 7) // 8),
                          "samples": st[0]["samples"], "wall_ms_median": round(1e3 * statistics.median(sec), 3),
                          "wall_ms_min_max": [round(1e3 * min(sec), 3), round(1e3 * max(sec), 3)],
                          "kernel_ms_median": round(statistics.median(s["kernel_ms"] for s in st), 3),
                          "kernel_used": st[0]["kernel_used"], "launches": st[0]["launches"], "repeats": a.repeats}))


if __name__ == "__main__":
    main()
