"""Scenes with nested Transforms (a Transform whose child is, or contains, another Transform), built on both builders -- rtamd.World and
the oracle's Scene share the reference's constructor names -- for tests/test_nested_transforms*.py.  Each builder returns a finished
scene: (rtamd.World, rtamd.Camera) for the product, an oracle.Scene with its camera (and shutter) set for the oracle."""
import numpy as np

from rtamd import shapes

CORNELL_CAM = ((278.0, 278.0, -800.0), (278.0, 278.0, 278.0), (0.0, 1.0, 0.0), 50.0, 1.5, 0.0, 10.0)
MAX_DEPTH = 8  # XF_MAX_DEPTH (common/flat.h)


def is_oracle(B):
    return not hasattr(B, "XZRectLight")


def bvh(B, ids, seed=1):
    return B.BVHNode_new(ids, seed) if is_oracle(B) else B.BVHNode_new(ids, bvh_seed=seed)


def nest(B, levels, obj):
    """levels: [(rotate, scale, translate)] innermost first -> Transform(..Transform(obj)..)"""
    for rot, sc, tr in levels:
        obj = B.Transform(rot, sc, tr, obj)
    return obj


def finish(B, items, seed=1, lights=(), cam=CORNELL_CAM, shutter=None):
    if is_oracle(B):
        B.World(items, seed)
        if lights:
            B.set_lights(list(lights), flux=[(1.0, 1.0, 1.0)] * len(lights), scale=[1000000.0] * len(lights))
        B.Camera(*cam)
        if shutter is not None:
            B.set_shutter(*shutter)
        return B
    import rtamd
    B.new(items, lights=lights, bvh_seed=seed)
    f, t, up, vfov, asp, ap, fd = cam
    return B, rtamd.Camera((f, t), up, vfov, asp, ap, fd)


def light(B):
    """XZRectLight::new (light.rs:134-146) as scene.rs:26-32 places it: flux (1, 1, 1), scale 1e6"""
    if is_oracle(B):
        return B.XZRectangle((213.0, 227.0), (343.0, 332.0), 554.0, B.DiffuseLight(B.ConstantTexture((1.0, 1.0, 1.0))))
    return B.XZRectLight((213.0, 227.0), (343.0, 332.0), 554.0, (1.0, 1.0, 1.0), 1000000.0)


def walls(B):
    red = B.Lambertian(B.ConstantTexture((0.75, 0.25, 0.25)))
    white = B.Lambertian(B.ConstantTexture((0.75, 0.75, 0.75)))
    blue = B.Lambertian(B.ConstantTexture((0.25, 0.25, 0.75)))
    return white, [
        B.YZRectangle((0.0, 0.0), (555.0, 555.0), 555.0, red),
        B.YZRectangle((0.0, 0.0), (555.0, 555.0), 0.0, blue),
        B.XZRectangle((0.0, 0.0), (555.0, 555.0), 0.0, white),
        B.XZRectangle((0.0, 0.0), (555.0, 555.0), 555.0, white),
        B.XYRectangle((0.0, 0.0), (555.0, 555.0), 555.0, white),
    ]


def n1(B):
    """Cornell box: each box is Transform(Transform(cube)); both sit under an outer rotate + translate Transform of a BVHNode"""
    white, items = walls(B)
    box1 = nest(B, [((0.0, 0.0, 0.0), (1.0, 2.0, 1.0), (0.0, 0.0, 0.0)), ((0.0, 15.0, 0.0), (1.0, 1.0, 1.0), (265.0, 0.0, 295.0))],
                B.Cube((0.0, 0.0, 0.0), (82.5, 82.5, 82.5), white))
    box2 = nest(B, [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((0.0, -18.0, 0.0), (1.0, 1.0, 1.0), (130.0, 0.0, 65.0))],
                B.Cube((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white))
    group = B.Transform((0.0, 4.0, 0.0), (1.0, 1.0, 1.0), (10.0, 0.0, -12.0), bvh(B, [box1, box2], 2))
    lt = light(B)
    return finish(B, items + [lt, group], lights=[lt])


def n2(B, nu=16, nv=32):
    """shapes.torus under 3 levels of rotation (all axes) and non-uniform scale, in the Cornell box"""
    white, items = walls(B)
    P, N, I = shapes.torus(nu, nv)
    mesh = B.Mesh(P, N, I, white, 3) if is_oracle(B) else B.Mesh(P, N, I, white, bvh_seed=3)
    t = nest(B, [((30.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((0.0, 45.0, 0.0), (1.5, 0.7, 1.2), (0.0, 0.5, 0.0)),
                 ((0.0, 0.0, 20.0), (100.0, 100.0, 100.0), (278.0, 250.0, 278.0))], mesh)
    lt = light(B)
    return finish(B, items + [lt, t], lights=[lt])


def n3(B):
    """one inner Transform object shared by two different outer Transforms, and also placed at world level"""
    white, items = walls(B)
    metal = B.Metal(B.ConstantTexture((0.8, 0.85, 0.88)), 0.1)
    inner = B.Transform((0.0, 30.0, 0.0), (1.0, 1.0, 1.0), (40.0, 0.0, 40.0), B.Cube((0.0, 0.0, 0.0), (80.0, 120.0, 80.0), white))
    ball = B.Transform((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 60.0, 0.0), B.Sphere((0.0, 0.0, 0.0), 40.0, metal))
    o1 = B.Transform((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (150.0, 0.0, 200.0), bvh(B, [inner, ball], 1))
    o2 = B.Transform((20.0, -40.0, 10.0), (1.5, 1.2, 1.5), (330.0, 120.0, 300.0), bvh(B, [inner, ball], 1))
    lt = light(B)
    return finish(B, items + [lt, o1, o2, inner, ball], lights=[lt])


def n4(B):
    """mixed depths 0-4 of spheres, rectangles and cubes in one BVH, with a 1-object BVHNode leaf over a Transform (Q14)"""
    white, items = walls(B)
    glass = B.Dielectric(1.5, B.ConstantTexture((0.999, 0.999, 0.999)))
    red = B.Lambertian(B.ConstantTexture((0.7, 0.3, 0.2)))
    L = [((0.0, 20.0, 0.0), (1.0, 1.0, 1.0), (10.0, 0.0, 0.0)), ((10.0, 0.0, 5.0), (1.1, 0.9, 1.0), (0.0, 5.0, 0.0)),
         ((0.0, 0.0, -15.0), (1.0, 1.0, 1.0), (0.0, 0.0, 10.0)), ((0.0, -10.0, 0.0), (0.9, 1.0, 1.1), (5.0, 0.0, 0.0))]
    objs = [
        B.Sphere((100.0, 60.0, 150.0), 60.0, glass),                                                       # depth 0
        nest(B, L[:1], B.XYRectangle((300.0, 20.0), (420.0, 160.0), 400.0, red)),                         # 1
        nest(B, L[:2], B.Cube((350.0, 0.0, 100.0), (450.0, 100.0, 200.0), white)),                        # 2
        nest(B, L[:3], B.Sphere((250.0, 300.0, 300.0), 50.0, red)),                                        # 3
        nest(B, L[:4], B.Cube((150.0, 0.0, 300.0), (230.0, 200.0, 380.0), white)),                        # 4
        bvh(B, [nest(B, L[:2], B.Sphere((420.0, 350.0, 250.0), 45.0, glass))], 5),                        # 1-object leaf (Q14), depth 2
    ]
    lt = light(B)
    return finish(B, items + [lt, bvh(B, objs, 4)], lights=[lt])


def n5(B):
    """a moving sphere and a noise texture at depth 2, shutter open"""
    white, items = walls(B)
    marble = B.Lambertian(B.NoiseTexture(0.05))
    L = [((0.0, 25.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 10.0), (1.2, 0.8, 1.0), (20.0, 10.0, 0.0))]
    ms = nest(B, L, B.MovingSphere((200.0, 200.0, 250.0), (240.0, 200.0, 250.0), 0.0, 1.0, 60.0, white))
    ns = nest(B, L, B.Sphere((380.0, 120.0, 250.0), 90.0, marble))
    lt = light(B)
    return finish(B, items + [lt, ms, ns], lights=[lt], shutter=(0.0, 1.0))


def n6(B):
    """a ConstantMedium under two Transforms, and a medium whose boundary is a depth-2 Transform"""
    white, items = walls(B)
    L = [((0.0, 15.0, 0.0), (1.0, 1.2, 1.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, -8.0), (1.0, 1.0, 1.0), (30.0, 0.0, 20.0))]
    fog1 = nest(B, L, B.ConstantMedium(0.01, B.Cube((120.0, 0.0, 80.0), (260.0, 200.0, 220.0), white), B.Isotropic(B.ConstantTexture((0.2, 0.2, 0.2)))))
    fog2 = B.ConstantMedium(0.008, nest(B, L, B.Sphere((380.0, 150.0, 330.0), 110.0, white)), B.Isotropic(B.ConstantTexture((0.9, 0.9, 0.9))))
    lt = light(B)
    return finish(B, items + [lt, fog1, fog2], lights=[lt])


def chain(levels):
    """levels of (rotate, scale, translate) with rotations about all axes and non-uniform scales, outermost last"""
    out = []
    for k in range(levels):
        rot = ((7.0 * k) % 40 - 20.0, (13.0 * k) % 50 - 25.0, (5.0 * k) % 30 - 15.0)
        sc = (1.0 + 0.05 * (k % 3), 1.0 - 0.04 * (k % 2), 1.0 + 0.03 * (k % 4))
        tr = (3.0 * k, -2.0 * k, 1.5 * k)
        out.append((rot, sc, tr))
    return out


def n7(B, levels=MAX_DEPTH):
    """a chain at the maximum depth: a cube and a sphere under `levels` Transforms"""
    white, items = walls(B)
    metal = B.Metal(B.ConstantTexture((0.8, 0.6, 0.5)), 0.05)
    grp = bvh(B, [B.Cube((-60.0, -60.0, -60.0), (60.0, 60.0, 60.0), white), B.Sphere((100.0, 80.0, 0.0), 50.0, metal)], 1)
    t = nest(B, chain(levels - 1) + [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (278.0, 200.0, 278.0))], grp)
    lt = light(B)
    return finish(B, items + [lt, t], lights=[lt])


def tie(B):
    """two cubes sharing the face x = 200: one at depth 1, one at depth 3"""
    white = B.Lambertian(B.ConstantTexture((0.75, 0.75, 0.75)))
    red = B.Lambertian(B.ConstantTexture((0.75, 0.25, 0.25)))
    a = B.Transform((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (100.0, 0.0, 0.0), B.Cube((0.0, 0.0, 0.0), (100.0, 100.0, 100.0), white))
    b = nest(B, [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (50.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (100.0, 0.0, 0.0)),
                 ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (50.0, 0.0, 0.0))], B.Cube((0.0, 0.0, 0.0), (100.0, 100.0, 100.0), red))
    return finish(B, [a, b], cam=((150.0, 50.0, -300.0), (200.0, 50.0, 50.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 10.0))


def tie_rays(n=4096, seed=7):
    """rays from inside either cube aimed at points of the shared face x = 200 (and a few through its edges)"""
    rng = np.random.default_rng(seed)
    tgt = np.stack([np.full(n, 200.0), rng.uniform(-5.0, 105.0, n), rng.uniform(-5.0, 105.0, n)], axis=1)
    side = rng.integers(0, 2, n)
    org = np.stack([np.where(side == 0, rng.uniform(110.0, 190.0, n), rng.uniform(210.0, 290.0, n)), rng.uniform(5.0, 95.0, n),
                    rng.uniform(5.0, 95.0, n)], axis=1)
    return np.concatenate([org, tgt - org], axis=1)


SCENES = {"n1": n1, "n2": n2, "n3": n3, "n4": n4, "n5": n5, "n6": n6, "n7": n7}
