"""What the ambient-occlusion pass (rt_ao_render) costs on one GPU: kernel_ms of one frame on the headline scene
(scene_500) and on the Cornell box with the 102,400-triangle mesh (tools/configs.py "c4"), through the accel walk and, with --kernel 1,
the reference-order walk.  After one warm-up call the frame is rendered --repeats times; one JSON line per scene gives the median, the
smallest and the largest kernel_ms, and a checksum of the frame (the same for every build that answers the same question).
An A/B build is measured by naming it in RTAMD_LIB (tools/build_variant.sh ao_closest -DRT_AO_CLOSEST_HIT: the occlusion rays go
through the closest-hit walks); alternate the builds in one job, a fresh process each.
  python tools/ao_run.py [--scenes scene_500 c4] [--width W] [--height H] [--ao-spp N] [--rays K] [--repeats R] [--kernel 0|1|2] [--label NAME]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402
import rtamd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["scene_500", "c4"])
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--ao-spp", type=int, default=4)
    ap.add_argument("--rays", type=int, default=4)
    ap.add_argument("--max-distance", type=float, default=float("inf"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--label", default=os.path.basename(rtamd.LIB_PATH))
    a = ap.parse_args()
    if rtamd.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    for key in a.scenes:
        world, cam = configs.product(key)
        kw = dict(ao_spp=a.ao_spp, rays_per_hit=a.rays, max_distance=a.max_distance, seed=1, kernel=a.kernel)
        frame, st = world.render_ao(cam, a.width, a.height, **kw)      # warm-up: uploads the scene
        ms = []
        for _ in range(a.repeats):
            ms.append(world.render_ao(cam, a.width, a.height, **kw)[1]["kernel_ms"])
        print(json.dumps({"build": a.label, "scene": key, "width": a.width, "height": a.height, "ao_spp": a.ao_spp, "rays_per_hit": a.rays,
                          "kernel_used": st["kernel_used"], "kernel_ms_median": round(statistics.median(ms), 3),
                          "kernel_ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "repeats": a.repeats,
                          "mean_visibility": float(frame[..., 0].mean()), "frame_sha16": hashlib.sha256(frame.tobytes()).hexdigest()[:16]}), flush=True)


if __name__ == "__main__":
    main()
