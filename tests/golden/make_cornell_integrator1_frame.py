"""Record tests/golden/cornell_32x32_4spp_seed1_integrator1.npy: the Cornell box (bvh_seed 1, aspect 1) under integrator 1 at 32 x 32,
4 spp, seed 1, rendered by the CPU oracle.  The committed file was written by the oracle of the commit before it learned backgrounds, env
sampling and area lights; tests/test_oracle_lights.py holds today's oracle to it.  Run from the repository root; needs no device."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle  # noqa: E402

o = oracle.cornell_box_scene(os.path.join(ROOT, "tests", "golden", "scenes", "cube.obj"), 1.0, seed=1)
img, _ = o.render(32, 32, 4, seed=1, integrator=1)
np.save(os.path.join(ROOT, "tests", "golden", "cornell_32x32_4spp_seed1_integrator1.npy"), img)
