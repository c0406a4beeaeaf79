"""irradiance_kernel and the light-sampling functions it shares with the shading kernels
(sphere_sample_from, sphere_pdf, sample_infinite, d1_sample, inf_lookup, infinite_pdf) against the
CPU oracle at light placements the shipped scenes never reach: a distance ladder from the light's
centre out to where the float 1 - ctmax is 0, the 1e-4 switch between cone and area sampling, radiance
maps with black runs, shadow segments that graze, start inside or end at an occluder, every material
branch of IrradianceTask, and the launch's edges. Scenes and points: tests/irradiance_hostile.py.

Criterion (irradiance_hostile.compare), per value: relative 1e-5 with no absolute floor (every term
of the estimator is non-negative: nothing cancels), exact zeros and non-finite values in the same
places, and per family >= 99 % of the values bit-identical. The figures are printed.

No sample of any family sends a ray with a NaN or infinite component into trace_any
(preprocess_kernels.hip irradiance_kernel, light_sample.h, geom.h):
  sphere light   wi = normalize(ps - p) and the segment direction (ps - p) / dist share their
                 divisor, so they are non-finite together; a trace needs nonblack = dot(ns, -wi) > 0,
                 which is false for a NaN wi (the point at ps == p, the NaN th of a cone sample whose
                 ct rounded above 1), and an infinite component needs |ps - p| < 1e-19 without being 0,
                 which float positions around a light of radius 0.5 cannot give. pdf = +inf (the far
                 rungs) leaves the ray finite. The point at the centre has wc = normalize(0), which
                 only the cone branch reads; it takes the area branch.
  infinite light the direction comes from uv alone, and Distribution1D's cdf is uniform where its
                 integral is 0 (montecarlo.h:68-71), so uv and wi are finite even on the all-black map,
                 whose pdfs are 0 / 0 = NaN; there the map lookup is black and the sample is dropped
                 before the trace.
"""
import os

import numpy as np
import pytest

import irradiance_hostile as ih
import oracle_render as orr
import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 8
ALBEDO = dict(texels=np.linspace(0.1, 0.9, 5 * 3 * 3, dtype=np.float32).reshape(3, 5, 3), gamma=2.2)
# material 0 has no BSSRDF (the ladder, shadow and launch families: Ft = 1, so the closed form applies)
MATERIALS = (ih.NO_BSSRDF, ih.SKIN, dict(ih.SKIN, albedo_tex=dict(ALBEDO, wrap="repeat")),
             dict(ih.SKIN, albedo_tex=dict(ALBEDO, wrap="clamp"), double_ref_sslf=1))


class Pair:
    """One scene on both sides; run(points, seed) -> (GPU irradiance, oracle irradiance)."""

    def __init__(self, mpss, lights, materials=(ih.NO_BSSRDF,), **cfg):
        from mpss import pbrtscene
        self.sc = ih.scene(lights, materials)
        self.replay = cfg.get("sampler") is not None
        self.ctx = pbrtscene.build_context(self.sc, **cfg)
        self.o = orr.OracleScene(self.sc, ih.irradiance_tables(self.sc, self.ctx), self.ctx.cfg, mpss)

    def run(self, pts, seed=7):
        self.ctx.set_surface_points(pts)
        self.ctx.preprocess(seed)
        got = self.ctx.irradiance()
        ref = (self.o.irradiance_replay(pts, cores=8, nthreads=NT) if self.replay
               else self.o.irradiance(pts, seed, nthreads=NT))
        return got, ref

    def close(self):
        self.o.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def one_sphere(mpss, oracle):
    import torch
    assert torch.cuda.is_available()
    p = Pair(mpss, [ih.sphere_light(64)], MATERIALS)
    yield p
    p.close()


def test_distance_ladder(one_sphere):
    pts, meta = ih.ladder_points()
    got, ref = one_sphere.run(np.concatenate([pts, ih.near_points()]))
    ih.compare(got, ref, "ladder")
    near = ih.near_points()
    cone = ~ih.switch_sides(near[9:], one_sphere.sc.lights[0])
    assert 10 <= cone.sum() <= len(cone) - 10     # both sides of the 1e-4 switch are in the family
    # the regimes on the GPU's own values (tests/test_irradiance_closed_form.py pins them on the oracle)
    L = ih.lemit_bands()
    facing = {rd: got[i].astype(np.float64) for i, (rd, j) in enumerate(meta) if j == 0}
    for rd in ih.LADDER:
        print("ladder R/d %g: E / disc = %.6g" % (rd, facing[rd][0] / (np.pi * L[0] * rd * rd)))
    for rd in (0.5, 0.1, 0.01):
        lo, hi, _ = ih.closed_form(rd, 0.0, L)
        assert np.all(facing[rd] >= lo) and np.all(facing[rd] <= hi), rd
    assert np.all(facing[1e-3] > 0)
    assert np.all(facing[1e-4] == 0) and np.all(facing[1e-5] == 0)


def test_closed_form_on_the_gpu(one_sphere):
    got, ref = one_sphere.run(ih.closed_form_points())
    ih.compare(got, ref, "closed form points")
    ih.check_closed_form(got)


def test_shadow_segments(one_sphere):
    got, ref = one_sphere.run(ih.shadow_points(), seed=3)
    ih.compare(got, ref, "shadow")
    assert np.all(ref[:6] == 0) and np.all(ref[8] > 0) and np.all(ref[9:11] == 0)   # the cases are what they claim
    assert 0.999 < ref[15, 0] / ref[18, 0] < 1.001                                   # triangle 2 occludes nothing


def _material_points():
    """Points of every material branch at R/d = 0.1 and 0.01, each with the normal facing the light
    (ct ~ 1), 0.1 % too long (ct > 1, clamped), square to it and nearly so (ct near 0) and in between:
    genprofile false (0); LayeredSkin, Ft from the rho table (1); LayeredSkin with an albedo texture
    looked up outside [0, 1], repeat (2) and clamp (3); material ids past the scene's (4, 2^32 - 1)."""
    recs = []
    u = ih._unit([0.3, -0.5, -0.8])
    side = ih._unit(np.cross(u, [0.3, 0.5, 0.8]))
    normals = [-u, -1.001 * u, side, ih._unit(side - 0.02 * u), ih._unit(-u + side)]
    k = 0
    for mat in (0, 1, 2, 3, 4, 0xFFFFFFFF):
        for d in (5.0, 50.0):
            for n in normals:
                k += 1
                p = u * d + side * 0.01 * k     # (at most 8 points may coincide: the octree's leaves)
                recs.append(ih.points([p], [n], material=mat, uv=[(-0.3, 1.7), (2.5, -1.2), (0.4, 0.6)][k % 3]))
    return np.concatenate(recs)


def test_material_branches(one_sphere):
    pts = _material_points()
    got, ref = one_sphere.run(pts, seed=5)
    ih.compare(got, ref, "material")
    m = pts["material"]
    lit = ref[:, 0] > 0
    assert all(lit[m == k].any() for k in np.unique(m))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_launch_edges(one_sphere, n):
    got, ref = one_sphere.run(ih.cloud(1000)[:n], seed=n)
    ih.compare(got, ref, "launch n=%d" % n)


@pytest.fixture(scope="module")
def one_sphere_replay(mpss, oracle):
    p = Pair(mpss, [ih.sphere_light(64)], MATERIALS, sampler=mpss.SAMPLER_REFERENCE, replay_cores=8)
    yield p
    p.close()


@pytest.mark.parametrize("n", [1, 7, 255, 256, 257, 1000])
def test_launch_edges_reference_sampler(one_sphere_replay, n):
    """The reference's own sampler: replay_irradiance_kernel deals the n points to 256 tasks, most of
    which own no point at these sizes."""
    got, ref = one_sphere_replay.run(ih.cloud(1000)[:n])
    ih.compare(got, ref, "replay n=%d" % n)


@pytest.mark.parametrize("ns,quick", [(1, 0), (3, 0), (64, 1)])
def test_sample_counts(mpss, oracle, ns, quick):
    """nsamples 1, 3 (RoundUpPow2: 4) and quick_render (nsamples / 4) on the ladder and the shadow family."""
    p = Pair(mpss, [ih.sphere_light(ns)], quick_render=quick)
    got, ref = p.run(np.concatenate([ih.ladder_points()[0], ih.near_points(), ih.shadow_points()]), seed=9)
    ih.compare(got, ref, "nsamples %d quick %d" % (ns, quick))
    p.close()


def _sky_points(li):
    """A cloud, plus points above the occluders whose normals face each pole of the map."""
    pole = np.asarray(li["l2w"], np.float64)[:3, :3] @ np.array([0.0, 0.0, 1.0])
    pts = ih.cloud(240, seed=8)
    extra = ih.cloud(16, seed=9)
    extra["n"][:8] = pole
    extra["n"][8:] = -pole
    return np.concatenate([pts, extra])


def test_three_lights(mpss, oracle):
    """Two sphere lights and an infinite light: the per-light scramble index 16 l."""
    sky = ih.sky_light(ih.sky_maps()["8x4hot"], nsamples=8)
    p = Pair(mpss, [ih.sphere_light(16), ih.sphere_light(4, centre=(2.0, -3.0, -1.0), radius=0.3, L=[5.0, 3.0, 1.0]), sky],
             MATERIALS)
    pts = np.concatenate([_sky_points(sky), _material_points(), ih.ladder_points()[0]])
    got, ref = p.run(pts, seed=11)
    ih.compare(got, ref, "three lights")
    # each light contributes: the whole differs from the one-sphere irradiance
    assert (ref[:, 0] > 0).mean() > 0.5
    p.close()


@pytest.mark.parametrize("name", ["none", "2x1", "8x4hot", "8x4black"])
def test_infinite_light_maps(mpss, oracle, name):
    sky = ih.sky_light(ih.sky_maps()[name], nsamples=64, L=(0.8, 0.9, 1.0))
    p = Pair(mpss, [sky])
    got, ref = p.run(_sky_points(sky), seed=13)
    ih.compare(got, ref, "sky " + name)
    if name == "8x4black":
        assert np.all(ref == 0)
    else:
        assert (ref[:, 0] > 0).mean() > 0.5
    p.close()


# ---------------------------------------------------------------- the same functions in the shading path
def _frame(mpss, lights, seed, min_dist=0.02, camera=None):
    """scenes/tissue.pbrt (a 1.2-wide slab in z = 0 with a block on it) at 32x32, 4 spp with its
    lights replaced: the scene, its surface points, the GPU film and the oracle film."""
    import torch
    from mpss import pbrtscene
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "tissue.pbrt"), xres=32, yres=32, spp=4)
    sc.integrator["minsampledistance"] = min_dist
    for m in sc.materials:
        m["desired_length"] = 128
    sc.lights = lights(sc)
    if camera is not None:
        sc.world_to_camera, sc.fov = camera
    ctx = pbrtscene.build_context(sc)
    ctx.preprocess(seed=seed)
    o = orr.OracleScene(sc, orr.tables_from_ctx(ctx, len(sc.materials)), ctx.cfg, mpss)
    pts = ctx.surface_points()
    E = o.irradiance(pts, seed, nthreads=NT)
    ih.compare(ctx.irradiance(), E, "frame irradiance")
    o.set_octree(pts, E)
    out = torch.zeros((sc.yres * sc.xres * 4,), dtype=torch.float32, device="cuda")
    ctx.render_tile(sc.spp, 17, 0, sc.xres, 0, sc.yres, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(sc.yres, sc.xres, 4)
    ref = o.render_tile(sc.spp, 17, 0, sc.xres, 0, sc.yres, nthreads=NT)
    o.close()
    ctx.close()
    return sc, pts, got, ref


TOUCH = np.array([-0.3, -0.2, 0.0])
TOUCH_LIGHT = dict(center=np.array([-0.3, -0.2, 0.05], np.float32), radius=0.05, L=[50.0, 50.0, 50.0], nsamples=4)


def touching_camera():
    """A camera 0.1 above the slab, 1 away from the point where the light touches it, half a degree
    wide: its rays pass under the sphere (a ray of elevation e clears a sphere of radius r down to
    e r / 2 = 2.5e-3 from the touching point) and meet the slab on either side of dist2 - r * r = 1e-4,
    which on the slab is the circle of radius 0.01 around that point."""
    from mpss import pbrtscene
    return pbrtscene.look_at([-0.3, -1.2, 0.1], TOUCH, [0, 0, 1]), 0.5


def test_touching_camera_sees_both_sides_of_the_switch():
    """(bookkeeping of the case itself; needs no device) pixel-centre rays meet the slab inside and
    outside the circle."""
    import synth
    from mpss import pbrtscene
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "tissue.pbrt"), xres=32, yres=32, spp=4)
    sc.world_to_camera, sc.fov = touching_camera()
    o, d = synth.pixel_centre_rays(sc)
    down = d[:, 2] < 0
    hit = o + d[down] * (-o[2] / d[down, 2])[:, None]
    h = np.linalg.norm(hit[:, :2] - TOUCH[:2], axis=1)
    assert ((h > 2e-3) & (h < 9e-3)).sum() >= 8 and ((h > 1.1e-2) & (h < 0.5)).sum() >= 8


def test_frame_touching_light(mpss, oracle):
    """A sphere light that touches the slab: surface points and camera hits fall on either side of
    the 1e-4 switch, and the MIS branch calls sphere_pdf there."""
    sc, pts, got, ref = _frame(mpss, lambda sc: [TOUCH_LIGHT], 6, min_dist=0.005, camera=touching_camera())
    near = ih.switch_sides(pts, TOUCH_LIGHT)
    assert near.sum() >= 4 and not near.all()
    parity.check_image(got, ref)


def test_frame_far_light(mpss, oracle):
    """A light at R/d = 1e-4: direct light and irradiance are exactly 0 (pdf = +inf). The frame is
    finite and equal to the oracle's."""
    far = dict(center=(ih._unit([0.11, 0.07, 1.0]) * 5000.0).astype(np.float32), radius=0.5, L=[4.0, 4.0, 4.0], nsamples=4)
    sc, pts, got, ref = _frame(mpss, lambda sc: [far], 6)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    assert np.array_equal(got[..., 3], ref[..., 3])
    assert np.array_equal(got[..., :3] == 0, ref[..., :3] == 0)
    nz = ref[..., :3] != 0
    if nz.any():   # (nothing but a ray that meets the light's sphere itself could carry light)
        rel = np.abs(got[..., :3][nz].astype(np.float64) - ref[..., :3][nz]) / np.abs(ref[..., :3][nz])
        assert rel.max() <= parity.TOL


def test_frame_black_row_sky(mpss, oracle):
    """Two sphere lights and the 8x4 sky with black rows and a black run of columns."""
    def lights(sc):
        second = dict(center=np.array([0.4, -0.5, 0.6], np.float32), radius=0.08, L=[300.0, 200.0, 100.0], nsamples=2)
        return [sc.lights[0], second, ih.sky_light(ih.sky_maps()["8x4hot"], nsamples=4)]
    sc, pts, got, ref = _frame(mpss, lights, 6)
    parity.check_image(got, ref)
