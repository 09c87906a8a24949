"""One BASELINE configuration (tools/configs.py) rendered N times in one process: the median, minimum and maximum kernel time, for
configurations whose launch is too short for tools/config_bench.py's single render to tell two builds apart (C1: 1.4 ms).
usage: [RTAMD_LIB=variants/librtamd_NAME.so] python tools/config_repeat.py [key] [N]   (default scene_10, 40) -> one JSON line"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

key = sys.argv[1] if len(sys.argv) > 1 else "scene_10"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
label, W, H, spp, _ = configs.CONFIGS[key]
world, cam = configs.product(key)
kw = dict(width=W, height=H, seed=1, integrator=configs.INTEGRATOR.get(key, 0), shutter=configs.SHUTTER.get(key, (0.0, 0.0)))
world.render(cam, spp=min(spp, 4), **kw)  # warm-up (workspace, code load)
ms = []
for _ in range(n):
    _, st = world.render(cam, spp=spp, **kw)
    ms.append(st["kernel_ms"])
ms = np.array(ms)
med = float(np.median(ms))
print(json.dumps({"lib": os.path.basename(os.environ.get("RTAMD_LIB", "librtamd.so")), "key": key, "renders": n, "kernel_ms_median": med, "min": float(ms.min()),
                  "max": float(ms.max()), "msamples_per_s_at_median": W * H * spp / (med * 1e-3) / 1e6, "kernel": st["kernel_used"], "lds": st["scene_in_lds"]}))
