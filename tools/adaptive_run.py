"""Tile-adaptive sampling (rt_render_adaptive) on one BASELINE configuration, one GPU: what it traces, what it costs and
what it buys.  Prints one JSON line per measurement:
  uniform      rt_render at the cap, `repeats` times, and its RMSE against the reference (the floor of every RMSE below)
  threshold_0  rt_render_adaptive with threshold 0 (bit-identical to the uniform frame: the cost of the ~log2(spp / min_spp) passes)
  adaptive     per threshold: samples traced, wall / kernel time, the histogram of tile spp, RMSE against the reference, and the RMSE of
               two uniform frames of the same cost: one that traces as many samples, one that takes as long (spp scaled by wall time)
The reference is a uniform frame at the cap with ANOTHER seed (--ref-seed): with the same seed a tile that runs to the cap would equal it
exactly and flatter the adaptive frame.  RMSE on linear radiance and on display values sqrt(clamp(c, 0, 1)) (the 8-bit conversion without
the quantisation).
usage: python tools/adaptive_run.py <config> [--spp N] [--min-spp N] [--thresholds a,b,c] [--kernel K] [--repeats R] [--ref-seed S]
configs: tools/configs.py (scene_500 = the headline, cornell = C3)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import configs  # noqa: E402


def rmse(a, b):
    d = a - b
    return float(np.sqrt(np.mean(d * d)))


def display(c):
    return np.sqrt(np.clip(c, 0.0, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--spp", type=int, default=0, help="the cap (default: the configuration's spp)")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--thresholds", default="0.01,0.02,0.03,0.05,0.1")
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ref-seed", type=int, default=2)
    a = ap.parse_args()
    label, W, H, spp_cfg, _ = configs.CONFIGS[a.config]
    spp = a.spp or spp_cfg
    world, cam = configs.product(a.config)
    integ = configs.INTEGRATOR.get(a.config, 0)
    kw = dict(seed=1, kernel=a.kernel, integrator=integ)
    world.render(cam, width=W, height=H, spp=2, **kw)  # warm-up: scene upload, code objects
    head = dict(config=a.config, label=label, width=W, height=H, spp=spp, min_spp=a.min_spp)
    ref = world.render(cam, width=W, height=H, spp=spp, **dict(kw, seed=a.ref_seed))[0]
    ref_d = display(ref)
    cap_seconds = []
    uni = None
    for r in range(a.repeats):
        uni, st = world.render(cam, width=W, height=H, spp=spp, **kw)
        cap_seconds.append(st["seconds"])
        print(json.dumps(dict(head, run="uniform", repeat=r, seconds=st["seconds"], kernel_ms=st["kernel_ms"], samples=st["samples"],
                              kernel_used=st["kernel_used"], rmse_linear=rmse(uni, ref), rmse_display=rmse(display(uni), ref_d))), flush=True)
    cap_s = min(cap_seconds)
    for r in range(a.repeats):
        img, tile_spp, st = world.render_adaptive(cam, W, H, spp, min_spp=a.min_spp, threshold=0.0, **kw)
        print(json.dumps(dict(head, run="threshold_0", repeat=r, seconds=st["seconds"], kernel_ms=st["kernel_ms"], samples=st["samples"],
                              launches=st["launches"], bit_identical=bool(np.array_equal(img, uni)))), flush=True)

    def uniform_at(n):
        n = max(1, min(spp, int(round(n))))
        f, st = world.render(cam, width=W, height=H, spp=n, **kw)
        return dict(spp=n, seconds=st["seconds"], rmse_linear=rmse(f, ref), rmse_display=rmse(display(f), ref_d))
    for thr in [float(t) for t in a.thresholds.split(",") if t]:
        img, tile_spp, st = world.render_adaptive(cam, W, H, spp, min_spp=a.min_spp, threshold=thr, **kw)
        vals, counts = np.unique(tile_spp, return_counts=True)
        print(json.dumps(dict(head, run="adaptive", threshold=thr, samples=st["samples"], sample_fraction=st["samples"] / float(W * H * spp),
                              seconds=st["seconds"], time_fraction=st["seconds"] / cap_s, kernel_ms=st["kernel_ms"], launches=st["launches"],
                              tile_spp_histogram={str(int(v)): int(c) for v, c in zip(vals, counts)},
                              rmse_linear=rmse(img, ref), rmse_display=rmse(display(img), ref_d),
                              equal_samples=uniform_at(st["samples"] / float(W * H)), equal_time=uniform_at(spp * st["seconds"] / cap_s))), flush=True)


if __name__ == "__main__":
    main()
