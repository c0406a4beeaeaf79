"""Synthetic scenes and surface points that put the lights where the shipped scenes never do
(tests/test_irradiance_closed_form.py on the CPU, tests/test_irradiance_hostile_gpu.py on the GPU).

Everything is laid out in a local frame (light 0 at its origin) and carried to the world by one
generic rotation and translation, so that no ray has a direction component of exactly 0 and no
ray starts on a bounding-box plane (the slab test's 0 * inf, tests/synth.py). The occluders live in
the half space z > 0 of that frame, the distance ladder in z < 0: nothing lies between a ladder
point and the light.

The occluder mesh (four triangles):
  0, 1  a quad in the plane z = 3 + 0.2 x over |x|, |y| <= 1, split along the diagonal through
        (0, 0, 3): the line from (0, 0, t) to the light's centre runs through that shared edge
  2     a 0.05-wide triangle square to G = (0.8, 0, 0.6), 1e-3 above the light's surface: for a
        point further out along G it lies inside the last 1e-3 of every shadow segment it crosses
  3     a triangle far off (it only gives the BVH an inner node)
"""
import numpy as np

from oracle_render import NB, SURFACE_POINT

R = 0.5                      # light 0's radius
LEMIT = [2.0, 2.0, 2.0]      # its Lemit (RGB)
CENTRE = np.array([0.3, -0.2, 0.4])
G = np.array([0.8, 0.0, 0.6])
LADDER = (0.98, 0.5, 0.1, 0.01, 1e-3, 5e-4, 3e-4, 2.5e-4, 2e-4, 1e-4, 1e-5)
_QUAD = np.array([[-1, -1, 2.8], [1, -1, 3.2], [1, 1, 3.2], [-1, 1, 2.8]], np.float64)
_QN = np.array([-0.2, 0.0, 1.0]) / np.sqrt(1.04)   # the quad's normal, away from the light


def _frame():
    from mpss import pbrtscene
    return (pbrtscene.rotate(37.0, [1, 2, 3]) @ pbrtscene.rotate(21.0, [-2, 1, 0.5]))[:3, :3]


def to_world(x):
    """Local points (n, 3) -> world."""
    return np.asarray(x, np.float64).reshape(-1, 3) @ _frame().T + CENTRE


def dir_world(v):
    return np.asarray(v, np.float64).reshape(-1, 3) @ _frame().T


def occluder_mesh():
    t1, t2 = np.array([0.6, 0.0, -0.8]), np.array([0.0, 1.0, 0.0])
    c0 = (R + 1e-3) * G
    small = [c0 + 0.05 * t1, c0 + 0.05 * (-0.5 * t1 + 0.87 * t2), c0 + 0.05 * (-0.5 * t1 - 0.87 * t2)]
    far = [[-9.0, 7.0, 5.0], [-8.0, 7.5, 5.5], [-8.5, 8.0, 4.5]]
    P = to_world(np.concatenate([_QUAD, small, far])).astype(np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9]], np.int32)
    o2w = np.eye(4, dtype=np.float32)
    return dict(P=P, N=None, S=None, uv=None, indices=idx, o2w=o2w, w2o=o2w.copy(), reverse=False, material=0)


NO_BSSRDF = dict(gen_profile=0)   # LayeredSkin with genprofile false: GetBSSRDF's data is NULL, Ft = 1, no albedo
SKIN = dict(roughness=0.3, nmperunit=40e6, Kr=[1.0, 1.0, 1.0], Kt=[0.0, 0.0, 0.0], layer_thickness_nm=[0.25e6, 20e6],
            layer_ior=[1.4, 1.4], f_mel=0.5, f_eu=0.5, f_blood=0.5, f_ohg=0.5, desired_length=64)


def sphere_light(nsamples=64, centre=(0, 0, 0), radius=R, L=LEMIT):
    return dict(center=to_world(centre)[0].astype(np.float32), radius=float(radius), L=list(L), nsamples=int(nsamples))


def sky_light(texels, nsamples=64, deg=52.0, axis=(1, -2, 0.7), L=(1.0, 1.0, 1.0)):
    from mpss import pbrtscene
    l2w = pbrtscene.rotate(deg, axis)
    li = dict(kind="infinite", L=list(L), scale=[1.0, 1.0, 1.0], nsamples=int(nsamples), l2w=l2w.astype(np.float32),
              w2l=np.linalg.inv(l2w).astype(np.float32))
    if texels is not None:
        li["texels"] = np.ascontiguousarray(texels, np.float32)
    return li


def sky_maps():
    """The radiance maps of the infinite-light family: none (the reference's 1x1 map), 2x1 with one
    black texel, 8x4 with black pole rows, a run of black columns and one hot texel, 8x4 all black
    (every Distribution1D has funcInt 0: its pdfs are 0 / 0, montecarlo.h:94)."""
    hot = np.zeros((4, 8, 3), np.float32)
    hot[1:3] = [0.2, 0.25, 0.3]
    hot[1:3, 4:7] = 0.0
    hot[1, 2] = [50.0, 40.0, 30.0]
    return {"none": None, "2x1": np.array([[[0.9, 0.7, 0.5], [0, 0, 0]]], np.float32), "8x4hot": hot,
            "8x4black": np.zeros((4, 8, 3), np.float32)}


def scene(lights, materials=(NO_BSSRDF,)):
    from mpss import pbrtscene
    sc = pbrtscene.Scene()
    sc.xres = sc.yres = 16
    sc.spp = 1
    sc.fov = 40.0
    sc.world_to_camera = pbrtscene.look_at(to_world([[0.5, -9.0, 2.0]])[0], CENTRE, [0.1, 0.2, 1.0])
    sc.integrator = dict(maxdepth=5, maxerror=0.1, minsampledistance=0.05)
    sc.materials = [dict(m) for m in materials]
    sc.meshes = [occluder_mesh()]
    sc.lights = list(lights)
    return sc


def irradiance_tables(sc, ctx=None):
    """Material tables for an irradiance-only comparison: IrradianceTask reads rho_hd alone (Ft,
    multipolesubsurface.cpp:121-123), so the Rd profile is left at zero. rho_hd comes from the
    context (ctx.material_tables); a genprofile-false material reads nothing."""
    out = []
    for i, m in enumerate(sc.materials):
        rho = np.zeros(2, np.float32) if not m.get("gen_profile", 1) else np.ascontiguousarray(
            ctx.material_tables(i)[2], np.float32)
        out.append((np.zeros((NB, 2), np.float32), np.ones(NB, np.float32), rho))
    return out


def points(p_local, n_local, material=0, ray_eps=1e-3, uv=(0.5, 0.5)):
    """SURFACE_POINT records from local positions and normals (broadcast against each other)."""
    p = to_world(p_local)
    n = dir_world(n_local)
    k = max(len(p), len(n))
    out = np.zeros(k, SURFACE_POINT)
    out["p"] = np.broadcast_to(p, (k, 3))
    out["n"] = np.broadcast_to(n, (k, 3))
    out["material"] = material
    out["ray_eps"] = ray_eps
    out["u"], out["v"] = uv
    out["area"] = 1e-4
    return out


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


_LADDER_DIRS = [_unit(v) for v in ([0.0, 0.0, -1.0], [0.6, 0.1, -0.8], [-0.2, -0.6, -0.75])]


def three_normals(u):
    """Facing the light's centre (which lies along -u from the point), square to it (the horizon
    cuts the cone of directions in half), and facing away."""
    side = _unit(np.cross(u, [0.3, 0.5, 0.8]))
    return [-u, side, u]


def ladder_points(rungs=LADDER, theta=None):
    """The distance ladder: for each R/d one point at distance d from light 0's centre with three
    normals (three_normals), or with the one normal at angle theta to the centre's direction."""
    recs, meta = [], []
    for k, rd in enumerate(rungs):
        u = _LADDER_DIRS[k % 3]
        p = u * (R / rd)
        if theta is None:
            ns = three_normals(u)
        else:
            side = _unit(np.cross(u, [0.3, 0.5, 0.8]))
            ns = [np.cos(theta) * -u + np.sin(theta) * side]
        for j, n in enumerate(ns):
            recs.append(points([p], [n]))
            meta.append((rd, j))
    return np.concatenate(recs), meta


def near_points():
    """The point at the centre, one inside, one on the surface (float32 rounding leaves it within an
    ulp of it), and 41 points whose dist2 - r * r steps ulp by ulp through the 1e-4 at which
    Sphere::Sample switches from the cone to the whole sphere (sphere.cpp:237): whatever the order a
    side sums dist2 in, some of them fall on either side of it. Three normals each (the centre:
    three fixed ones)."""
    recs = []
    for n in ([0, 0, 1.0], [0.6, 0, -0.8], [0, -1.0, 0]):
        recs.append(points([[0, 0, 0]], [n]))
    u = _LADDER_DIRS[1]
    for d in (0.2, R):
        for n in three_normals(u):
            recs.append(points([u * d], [n]))
    d0 = np.sqrt(R * R + 1e-4)
    u = _LADDER_DIRS[2]
    for k in range(-20, 21):
        d = d0 * (1.0 + k * 2.0 ** -25 / (2 * 0.2501))   # one ulp of dist2 (2^-25 in [0.25, 0.5)) per step
        for n in three_normals(u):
            recs.append(points([u * d], [n]))
    return np.concatenate(recs)


def switch_sides(pts, light):
    """dist2 - r * r < 1e-4 per point, in float32 with the sum taken left to right."""
    f = np.float32
    d = pts["p"].astype(f) - np.asarray(light["center"], f)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r = f(light["radius"])
    return (d2 - r * r) < f(1e-4)


def shadow_points():
    """The shadow-segment family (see the module docstring for the occluders)."""
    recs = []
    x_on = np.array([0.3, -0.4, 3.06])               # on the quad, off its diagonal
    for t in (6.0, 12.0):                            # the quad's shared edge lies through the line to the centre
        for n in three_normals(_unit([0, 0, 1.0])):
            recs.append(points([[0, 0, t]], [n]))
    recs.append(points([[2.0, 0.0, 6.4]], [_unit([-2.0, 0, -6.4])]))      # the line crosses an outer edge's midpoint
    recs.append(points([[2.0, 0.0, 6.4]], [_unit([1.0, 0.2, -0.1])]))
    for eps in (1e-3, 1e-5, 0.0):                    # 1e-4 behind the quad: inside ray_eps, beyond it, ray_eps 0
        recs.append(points([x_on + 1e-4 * _QN], [-_QN], ray_eps=eps))
    for eps in (1e-3, 0.0):                          # in the occluder's plane: on the quad itself ...
        recs.append(points([x_on], [-_QN], ray_eps=eps))
    for p in ([2.5, 0.3, 3.5], [-3.0, 0.5, 2.4]):    # ... and beside it
        recs.append(points([p], [_unit(-np.asarray(p))]))
    for t, eps in ((6.0, 1e-3), (60.0, 1e-3), (0.9, 1e-5)):   # triangle 2: inside the last 1e-3 (twice), and not
        recs.append(points([G * t], [-G], ray_eps=eps))
    for p in ([0, 0, 6.0], [-3.0, 2.0, 1.0]):        # ray_eps beyond the light: nothing can occlude
        recs.append(points([p], [_unit(-np.asarray(p))], ray_eps=100.0))
    recs.append(points([[-3.0, 2.0, 1.0]], [_unit([3.0, -2.0, -1.0])], ray_eps=0.0))
    return np.concatenate(recs)


def cloud(n, seed=5):
    """n distinct points around the occluders and the light, normals roughly towards light 0 (a
    fifth of them anywhere), ray_eps over four decades."""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform([-3, -3, 0.8], [3, 3, 7], (n - n // 3, 3)),
                        rng.uniform([-4, -4, -6], [4, 4, -0.8], (n // 3, 3))])[rng.permutation(n)]
    nr = -p / np.linalg.norm(p, axis=1, keepdims=True) + 0.6 * rng.standard_normal((n, 3))
    anyw = rng.random(n) < 0.2
    nr[anyw] = rng.standard_normal((int(anyw.sum()), 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    out = points(p, nr)
    out["ray_eps"] = 10.0 ** rng.uniform(-6, -2, n)
    return out


# ---------------------------------------------------------------- the closed form
def lemit_bands():
    import mpss
    return mpss.host_from_rgb(LEMIT).astype(np.float64)


def closed_form(rd, theta, L, rounding=True):
    """(lo, hi, disc) per band in float64 for an unoccluded point without a BSSRDF. alpha =
    asin(R/d); every estimator term is L Omega cos(theta_i) with Omega = 2 pi (1 - cos alpha) and
    theta_i in [theta - alpha, theta + alpha], so E lies in L Omega [cos(theta + alpha), max cos]:
    max cos is cos(theta - alpha), or 1 when that interval of angles contains 0 (theta < alpha; the
    bracket would otherwise shrink to one value that excludes the disc formula). Widened by the
    rounding of the float 1 - ctmax, relative 2^-23 / (1 - cos alpha) (left out with rounding=False:
    the bracket of exact arithmetic), plus 1e-5. disc = pi L (R/d)^2 cos theta lies inside."""
    a = np.arcsin(rd)
    assert theta + a < np.pi / 2
    om = 2.0 * np.pi * (1.0 - np.cos(a))
    w = (2.0 ** -23 / (1.0 - np.cos(a)) if rounding else 0.0) + 1e-5
    lo = L * om * np.cos(theta + a) * (1.0 - w)
    hi = L * om * np.cos(max(0.0, theta - a)) * (1.0 + w)
    disc = np.pi * L * rd * rd * np.cos(theta)
    assert np.all(lo <= disc) and np.all(disc <= hi)
    return lo, hi, disc


CLOSED_FORM_CASES = [(rd, th) for rd in (0.5, 0.2, 0.1, 0.02) for th in (0.0, 0.7)]


def closed_form_points():
    recs = []
    for rd, th in CLOSED_FORM_CASES:
        recs.append(ladder_points([rd], theta=th)[0])
    return np.concatenate(recs)


def check_closed_form(E):
    """E: irradiance of closed_form_points() under sphere_light(64) alone."""
    L = lemit_bands()
    for (rd, th), e in zip(CLOSED_FORM_CASES, np.asarray(E, np.float64)):
        lo, hi, _ = closed_form(rd, th, L)
        assert np.all(e >= lo) and np.all(e <= hi), (rd, th, float((e / lo).min()), float((e / hi).max()))


# ---------------------------------------------------------------- the criterion
def compare(got, ref, name):
    """Per value: relative 1e-5 with no absolute floor, the exact zeros and the non-finite values in
    the same places; per family at least 99 % of the values bit-identical. Prints the figures."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    same = got.view(np.uint32) == ref.view(np.uint32)
    fin = np.isfinite(ref)
    nz = fin & (ref != 0)
    g, r = got.astype(np.float64), ref.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(g - r)[nz] / np.abs(r[nz])
    worst = float(rel.max()) if rel.size else 0.0
    print("%s: %d values, %d zero, %d non-finite, bit-identical %.4f, max rel %.3g"
          % (name, ref.size, int((ref == 0).sum()), int((~fin).sum()), same.mean(), worst))
    assert np.array_equal(got == 0, ref == 0), "%s: exact zeros differ" % name
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), \
        "%s: non-finite values differ" % name
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    assert np.all(np.isfinite(got[nz])) and worst <= 1e-5, "%s: relative difference %g" % (name, worst)
    assert same.mean() >= 0.99, "%s: bit-identical share %.4f" % (name, same.mean())
    return same.mean(), worst
