"""Record tests/golden/env_sampling_off_frames.json: the SHA-256 of the f64 frames that tests/test_env_sampling_gpu.py's off_frames()
renders WITHOUT env sampling (Cornell + sky under integrator 1; the open scene of tests/test_background_gpu.py under the sky).  Run on a
GPU against a build of the commit BEFORE env sampling existed, so that the test proves that a scene which leaves the switch off kept
its frames:
    python tests/golden/make_env_sampling_off_frames.py --package DIR [--out FILE]
DIR holds that commit's `rtamd` package and librtamd.so (default: this tree's rust-raytracer_amd)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--package", default=os.path.join(ROOT, "rust-raytracer_amd"))
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "env_sampling_off_frames.json"))
ap.add_argument("--commit", default="", help="the commit the package was built from (recorded in the file)")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.package))
import rtamd  # noqa: E402  (first: the test module's imports then find this one)

assert os.path.dirname(os.path.abspath(rtamd.__file__)).startswith(os.path.abspath(a.package))
sys.path.insert(1, os.path.join(ROOT, "tests"))
import test_env_sampling_gpu as t  # noqa: E402

frames = t.off_frames()
json.dump({"recorded_on": a.commit, "what": "sha256 of the f64 frame bytes, env sampling off (test_env_sampling_gpu.off_frames)", "frames": frames},
          open(a.out, "w"), indent=1, sort_keys=True)
print(json.dumps(frames, indent=1, sort_keys=True))
