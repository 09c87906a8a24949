"""The small sphere scenes of the START walks' tests: tests/test_walk_start.py asks the start rule about each without a
device, tests/test_walk_start_gpu.py renders them.  A sphere is (centre, radius, material key); EXPECT says what the rule does with the
root of the scene's tree: "ground" = the walk starts at a leaf that holds the radius-1000 sphere alone, "pair" = at a leaf of two items
(the ground and its coincident twin: equal centroids are never split), "root" = at the root, as ever."""

GROUND = ((0.0, -1000.0, 0.0), 1000.0, "gray")
TWIN = ((0.0, -1000.0, 0.0), 1000.0, "mirror")       # the ground sphere again, another material: every hit of one is an exact tie with the other
SMALL_GROUND = ((0.0, -1.5, 0.0), 1.5, "gray")
LAMP = ((2.5, 15.0, 1.0), 2.0, "light")              # far enough above the rest to be a leaf child of the root beside a small ground
GLASS = ((-2.2, 0.7, 0.3), 0.7, "glass")
BALL = ((0.0, 1.0, 0.0), 1.0, "mirror")
LIT = ((2.2, 0.7, -0.3), 0.7, "light")                # a light in the camera's view: without one most paths end black
GLOW = ((0.0, 1.0, 0.0), 1.0, "light")

SCENES = {
    "five": [GROUND, LAMP, GLASS, BALL, LIT],                # ratio 0.994: the rule picks the ground leaf
    "five_small": [SMALL_GROUND, LAMP, GLASS, BALL, LIT],    # the root's leaf child is the lamp, 0.177 of the area: not picked
    "two": [GROUND, GLOW],                                   # two leaves under the root; the pushed ref is a leaf
    "one": [GLOW],                                           # the one-item BVH
    "tie_before": [TWIN, GROUND, LAMP, GLASS, LIT],
    "tie_after": [GROUND, LAMP, GLASS, LIT, TWIN],
}
EXPECT = {"five": "ground", "five_small": "root", "two": "ground", "one": "root", "tie_before": "pair", "tie_after": "pair"}

CAM = ((0.0, 1.4, 6.0), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0), 40.0, 16.0 / 9.0, 0.0, 10.0)


def build(B, name):
    """the scene's sphere handles through a builder B (rtamd.World or oracle.Scene: the same calls)"""
    mats = {
        "gray": lambda: B.Lambertian(B.ConstantTexture((0.5, 0.5, 0.5))),
        "blue": lambda: B.Lambertian(B.ConstantTexture((0.2, 0.3, 0.8))),
        "mirror": lambda: B.Metal(B.ConstantTexture((0.2, 0.9, 0.2)), 0.0),
        "glass": lambda: B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0))),
        "light": lambda: B.DiffuseLight(B.ConstantTexture((5.0, 5.0, 5.0))),
    }
    return [B.Sphere(c, r, mats[m]()) for c, r, m in SCENES[name]]
