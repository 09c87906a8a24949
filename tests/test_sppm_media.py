"""Oracle-only properties of SPPM on scenes with a ConstantMedium (the semantics rt_render_sppm follows bit for bit,
tests/test_sppm_media_gpu.py)."""
import numpy as np

CFG = dict(iterations=2, photons_per_iter=20000, k_global=30, k_caustic=10)
CAM = ((0.0, 4.0, -8.0), (0.0, 0.5, 0.0), (0, 1, 0), 40.0, 1.0, 0.0, 8.0)


def _scene(fog=None):
    """a floor and a sphere light; fog = (density, albedo, radius): a sphere-bounded fog around the light, no surface inside it"""
    import oracle
    o = oracle.Scene()
    white = o.Lambertian(o.ConstantTexture((0.8, 0.8, 0.8)))
    light = o.Sphere((0.0, 3.0, 0.0), 0.3, o.DiffuseLight(o.ConstantTexture((1.0, 1.0, 1.0))))
    items = [o.XZRectangle((-50.0, -50.0), (50.0, 50.0), 0.0, white), light]
    if fog is not None:
        density, albedo, radius = fog
        items.append(o.ConstantMedium(density, o.Sphere((0.0, 3.0, 0.0), radius, white), o.Isotropic(o.ConstantTexture((albedo,) * 3))))
    o.World(items, 1)
    o.set_lights([light], flux=[(1.0, 1.0, 1.0)], scale=[100.0])
    o.Camera(*CAM)
    return o


def test_a_thin_fog_stores_as_many_photons_as_the_clear_scene():
    """density 1e-9: (almost) no photon scatters, but every boundary crossing still draws once, so the streams -- and the photon
    sets -- differ from the clear scene's; the totals agree within sampling noise"""
    _, _, (g0, c0) = _scene().render_sppm(8, 8, 0, seed=3, n_workers=8, **CFG)
    _, _, (g1, c1) = _scene((1e-9, 0.9, 2.0)).render_sppm(8, 8, 0, seed=3, n_workers=8, **CFG)
    assert g0 > 1000 and (g0, c0) != (g1, c1)
    assert abs(g1 - g0) < 5.0 * np.sqrt(g0) + 0.02 * g0

