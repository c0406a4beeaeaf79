"""Seeded synthetic inputs shared by the parity tests and bench.py."""
import numpy as np

NB = 30


def smooth_spectra(n, seed=1, black_frac=0.0):
    """E_c = s * (0.5 + 0.5 sin(0.1 c + phi)), s ~ U[0,1)."""
    rng = np.random.default_rng(seed)
    s = rng.random(n, dtype=np.float32)
    phi = rng.random(n, dtype=np.float32) * np.float32(6.2831853)
    c = np.arange(NB, dtype=np.float32)
    E = (s[:, None] * (np.float32(0.5) + np.float32(0.5) * np.sin(np.float32(0.1) * c[None, :] + phi[:, None])))
    E = E.astype(np.float32)
    if black_frac > 0:
        E[rng.random(n) < black_frac] = 0.0
    return E


def ellipsoid_cloud(n, radii=(0.25, 0.3, 0.35), seed=7, black_frac=0.05):
    """Irradiance points on an ellipsoid surface: p, n, E, area."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = np.asarray(radii)
    p = (v * r).astype(np.float32)
    nrm = v / (r * r)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    area_total = 4 * np.pi * (np.prod(r) ** (2 / 3))
    area = np.full(n, area_total / n, np.float32) * (0.5 + rng.random(n).astype(np.float32))
    return p, nrm.astype(np.float32), smooth_spectra(n, seed + 1, black_frac), area.astype(np.float32)


def surface_queries(q, radii=(0.25, 0.3, 0.35), seed=11, jitter=0.0, sort=True):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((q, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    p = v * np.asarray(radii)
    if jitter:
        p += rng.standard_normal((q, 3)) * jitter
    p = p.astype(np.float32)
    if sort:  # Morton order: neighbouring queries share octree paths, like a pixel's samples
        p = p[np.argsort(morton3(p), kind="stable")]
    return np.ascontiguousarray(p)


def morton3(p, bits=10):
    """30-bit Morton code of points quantised over their bounding box."""
    lo = p.min(0)
    span = np.maximum(p.max(0) - lo, 1e-30)
    q = np.minimum(((p - lo) / span * (1 << bits)).astype(np.uint64), (1 << bits) - 1)
    code = np.zeros(len(p), np.uint64)
    for b in range(bits):
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return code


def texture_texels(w, h, seed=3, lo=0.05, hi=1.0):
    """A (h, w, 3) RGB image like a skin diffuse map: smooth colour bands plus per-texel noise,
    values in [lo, hi) (ReadImage's float texels)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([0.5 + 0.4 * np.sin(x / max(w, 1) * 6.3 + k + y / max(h, 1) * 2.1) for k in range(3)], -1)
    img = lo + (hi - lo) * np.clip(0.8 * base + 0.2 * rng.random((h, w, 3)), 0, 0.999)
    return img.astype(np.float32)


def random_uvd(n, seed=5, scale=0.02, outside=0.1):
    """(n, 6) lookup points u, v, dudx, dvdx, dudy, dvdy: u, v partly outside [0, 1) (wrap
    modes), differentials log-uniform over ~4 decades of `scale`, a share of them zero
    (the irradiance / tessellation lookups) and a share strongly anisotropic."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-outside, 1 + outside, (n, 2))
    d = rng.standard_normal((n, 4)) * scale * np.exp(rng.uniform(-4.5, 4.5, (n, 1)))
    d[rng.random(n) < 0.15] = 0.0
    an = rng.random(n) < 0.15
    d[an, 2:] *= 1e-3
    return np.concatenate([uv, d], 1).astype(np.float32)


# ---------------------------------------------------------------- hostile scenes for the BVH tracers
# (tests/test_trace_oracle.py on the CPU, tests/test_trace_gpu.py on the GPU)
#
# Each builder returns a pbrtscene.Scene made in memory: meshes as the dicts Scene documents, one
# LayeredSkin material (scenes/skin.pbrt's, desired_length 128), one sphere light and a camera, at
# most 4096 triangles, a 64x64 frame at 4 spp. sc.trace_eps is the distance a test's shadow rays
# start off their triangle; sc.min_dist the minsampledistance that gives a few thousand points.
#
# What stays out of every scene, and why: exactly coincident surfaces, and rays with a direction
# component of exactly 0. For such rays pbrt's slab test (which the product restates) has 0 * inf =
# NaN in it, and its answer then depends on the comparison order and on the tree; the oracle's padded,
# NaN-skipping boxes do not reproduce that. A closest-hit tie between two triangles at equal t is
# decided by the order the tree offers them in, which differs between two builders as well. Surfaces
# may come close (1e-4 of the scene) but their t along any ray stays apart by far more than a float's
# resolution.
FRAME = 64
_SKIN = dict(roughness=0.3, nmperunit=40e6, Kr=[1.0, 1.0, 1.0], Kt=[0.0, 0.0, 0.0], layer_thickness_nm=[0.25e6, 20e6],
             layer_ior=[1.4, 1.4], f_mel=0.5, f_eu=0.5, f_blood=0.5, f_ohg=0.5, desired_length=128)


def _mesh(P, idx):
    o2w = np.eye(4, dtype=np.float32)
    return dict(P=np.ascontiguousarray(P, np.float32).reshape(-1, 3), N=None, S=None, uv=None,
                indices=np.ascontiguousarray(idx, np.int32).reshape(-1, 3), o2w=o2w, w2o=o2w.copy(), reverse=False,
                material=0)


def _soup(tris):
    """(n, 3, 3) triangle soup -> one mesh with its own three vertices per triangle."""
    tris = np.asarray(tris, np.float32)
    return _mesh(tris.reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3))


def _scene(meshes, pos, look, up, fov, light, trace_eps, min_dist):
    from mpss import pbrtscene
    sc = pbrtscene.Scene()
    sc.xres = sc.yres = FRAME
    sc.spp = 4
    sc.fov = float(fov)
    sc.world_to_camera = pbrtscene.look_at(pos, look, up)
    sc.integrator = dict(maxdepth=5, maxerror=0.1, minsampledistance=float(min_dist))
    sc.materials = [dict(_SKIN)]
    sc.meshes = list(meshes)
    sc.lights = [dict(center=np.asarray(light[0], np.float32), radius=float(light[1]), L=[60.0, 60.0, 60.0],
                      nsamples=4)]
    sc.trace_eps = float(trace_eps)
    sc.min_dist = float(min_dist)
    assert sum(len(m["indices"]) for m in sc.meshes) <= 4096
    return sc


def scene_triangles(sc):
    """(n, 3, 3) float32 vertices of the scene's triangles in the global order both tracers number
    them by (meshes in scene order)."""
    return np.concatenate([np.asarray(m["P"], np.float32)[np.asarray(m["indices"])] for m in sc.meshes])


def pixel_centre_rays(sc):
    """Camera rays through the pixel centres, row-major: origin (3,), directions (yres * xres, 3),
    float32 and operation by operation as the tile-cost probe computes them (primary.hip
    probe_kernel: RasterToCamera of (x + .5, y + .5, 0), divided by w, normalised by a reciprocal,
    CameraToWorld as a vector)."""
    f = np.float32
    r2c, c2w = sc.raster_to_camera()
    ys, xs = np.mgrid[0:sc.yres, 0:sc.xres]
    px, py = (xs.ravel().astype(f) + f(0.5)), (ys.ravel().astype(f) + f(0.5))

    def point(m, x, y):  # Transform::operator()(Point) with z = 0: m*x + m*y + m*0 + m, left to right
        rows = [m[r, 0] * x + m[r, 1] * y + m[r, 2] * f(0) + m[r, 3] for r in range(4)]
        inv = f(1) / rows[3]
        one = rows[3] == f(1)
        return [np.where(one, rows[k], rows[k] * inv) for k in range(3)]

    cx, cy, cz = point(r2c, px, py)
    inv = f(1) / np.sqrt(cx * cx + cy * cy + cz * cz)
    cx, cy, cz = cx * inv, cy * inv, cz * inv
    d = np.stack([c2w[r, 0] * cx + c2w[r, 1] * cy + c2w[r, 2] * cz for r in range(3)], 1).astype(f)
    o = np.array([c2w[r, 3] for r in range(3)], f)  # CameraToWorld of the origin (w = 1)
    return o, np.ascontiguousarray(d)


def sign_octants(d):
    """dirIsNeg pattern per direction, as the packet tracer groups its lanes: bit k set when 1 / d[k] < 0."""
    neg = d < 0
    return neg[:, 0].astype(int) | (neg[:, 1].astype(int) << 1) | (neg[:, 2].astype(int) << 2)


def wave_octant_counts(sc, d):
    """Sign patterns per wave of the primary-ray kernel on the full frame at sc.spp: it numbers the
    samples pixel-major over the frame's rows (a full-frame tile's sample extent is the frame) with
    the pixel's spp samples adjacent, so a 64-lane wave holds 64 / spp consecutive pixels."""
    per = 64 // sc.spp
    assert 64 % sc.spp == 0 and (sc.xres * sc.yres) % per == 0
    pat = sign_octants(d).reshape(-1, per)
    return np.array([len(np.unique(p)) for p in pat])


def _shards(rng, n, lo, hi, keep_out, size=(2.5e-4, 0.25), sliver_frac=0.1):
    """n disjoint random triangles inside the box [lo, hi]: longest edges log-uniform over three
    decades, a share of them slivers of aspect ratio >= 1e3. keep_out: [(centre, radius)] spheres to
    stay clear of. Disjoint by construction: the bounding spheres do not meet (largest placed first)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    L = np.sort(np.exp(rng.uniform(np.log(size[0]), np.log(size[1]), n)))[::-1]
    cen = [np.asarray(c, np.float64) for c, _ in keep_out]
    rad = [float(r) for _, r in keep_out]
    out = []
    for Li in L:
        r = 0.5 * Li * 1.01
        for _ in range(200):
            c = rng.uniform(lo + r, hi - r)
            if len(cen) == 0 or np.all(np.linalg.norm(np.asarray(cen) - c, axis=1) > np.asarray(rad) + r):
                break
        else:
            raise AssertionError("shards: no room for a triangle of size %g" % Li)
        cen.append(c)
        rad.append(r)
        u = rng.standard_normal(3)
        u /= np.linalg.norm(u)
        v = np.cross(u, rng.standard_normal(3))
        v /= np.linalg.norm(v)
        # base along u (length Li, centred on c), apex off it by the height h along v
        sliver = rng.random() < sliver_frac
        h = Li * (rng.uniform(2e-4, 9e-4) if sliver else rng.uniform(0.3, 0.8))
        s = rng.uniform(-0.3, 0.3)
        out.append([c - 0.5 * Li * u, c + 0.5 * Li * u, c + s * Li * u + h * v])
    tris = np.asarray(out)
    return tris[rng.permutation(n)]


def triangle_aspects(tris):
    """Longest edge over the height on it, per triangle (float64)."""
    t = np.asarray(tris, np.float64)
    e = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]], 1)
    ln = np.linalg.norm(e, axis=2)
    area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
    return ln.max(1) ** 2 / area2, ln


def shard_cloud(seed=1, n=3000):
    """About 3000 disjoint shards in the box [-1, 1]^3 with the camera inside it at the origin,
    looking along (1, 1, 1) with a 150 degree field of view: the +x, +y and +z axis directions are
    in frame, so the frame's rays have 7 of the 8 sign patterns and the waves around an axis
    direction hold 3 or 4 of them."""
    rng = np.random.default_rng(seed)
    light = ([0.9, -2.2, 2.4], 0.3)
    tris = _shards(rng, n, [-1, -1, -1], [1, 1, 1], keep_out=[([0, 0, 0], 0.06)])
    sc = _scene([_soup(tris)], [0, 0, 0], [1, 1, 1], [0.1, 0.25, 1.0], 150.0, light, trace_eps=2e-5, min_dist=0.05)
    o, d = pixel_centre_rays(sc)
    assert np.all(d != 0), "a pixel-centre ray has a zero direction component"
    assert len(np.unique(sign_octants(d))) >= 7
    assert wave_octant_counts(sc, d).max() >= 3
    return sc


def stacked_sheets(seed=2, nsheets=8, grid=16):
    """8 parallel sheets of 16 x 16 jittered quads, 1e-4 of the scene's size (its bounding box) apart,
    tilted off every axis and seen at 30 degrees from their plane. Sheet k is mesh k; sheet 0 faces
    the camera and the light, and each sheet reaches 0.02 less far than the one in front of it, so
    from the camera and from the light sheet 0 covers all the others. The vertices are jittered inside
    the sheet's plane only (and each sheet by its own amounts): the sheets never meet. A two-triangle
    awning (the last mesh) shades part of the stack from the light."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.36, 0.48, 0.8])           # unit
    a = np.cross(nrm, [0.0, 0.0, 1.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    corners = np.array([[i, j] for i in (-1.0, 1.0) for j in (-1.0, 1.0)]) @ np.stack([a, b])
    gap = 1e-4 * np.ptp(corners, axis=0).max()
    meshes = []
    for k in range(nsheets):
        half = 1.0 - 0.02 * k
        g = np.linspace(-half, half, grid + 1)
        u, v = np.meshgrid(g, g, indexing="ij")
        jit = 0.3 * (2 * half / grid)
        inner = np.zeros_like(u, bool)
        inner[1:-1, 1:-1] = True
        u = u + inner * rng.uniform(-jit, jit, u.shape)
        v = v + inner * rng.uniform(-jit, jit, v.shape)
        P = u[..., None] * a + v[..., None] * b - (k * gap) * nrm
        i = np.arange(grid)[:, None] * (grid + 1) + np.arange(grid)[None, :]
        q = np.stack([i, i + grid + 1, i + grid + 2, i, i + grid + 2, i + 1], -1).reshape(-1, 3)
        if k == nsheets - 1:
            q = q[:-2]  # one quad less on the back sheet: room for the awning below within 4096 triangles
        meshes.append(_mesh(P.reshape(-1, 3), q))
    # 30 degrees above the sheet plane, along the in-plane direction a + b
    w = (a + b) / np.sqrt(2.0)
    pos = 2.6 * (np.cos(np.radians(30)) * w + np.sin(np.radians(30)) * nrm)
    light = (2.5 * nrm + 0.8 * a - 0.5 * b, 0.25)
    # the awning: a slightly tilted quad half a unit above the far side of the sheets (behind them as the
    # camera sees it, so it hides none of them), between the light and about a quarter of each sheet.
    # Preprocess starts its shadow rays minsampledistance / 10 off a point, which is beyond the whole
    # stack: the awning is what gives Preprocess's any-hit rays something to be blocked by here.
    wv = (a + b) / np.sqrt(2.0)
    uv = (a - b) / np.sqrt(2.0)
    aw = np.array([-1.25 * wv - 1.1 * uv + 0.5 * nrm, -0.2 * wv - 1.1 * uv + 0.56 * nrm,
                   -0.2 * wv + 1.1 * uv + 0.6 * nrm, -1.25 * wv + 1.1 * uv + 0.53 * nrm])
    meshes.append(_mesh(aw, [[0, 1, 2], [0, 2, 3]]))
    sc = _scene(meshes, pos, [0, 0, 0], nrm, 48.0, light, trace_eps=gap / 4, min_dist=0.12)
    sc.sheet_tris = 2 * grid * grid
    sc.n_sheet_tris = nsheets * 2 * grid * grid - 2  # the sheets' triangles; the awning's two follow
    sc.sheet_normal = nrm
    return sc


def _centred_triangle(rng, c, half):
    """A triangle whose bounding box is exactly c +- half (c, half on a dyadic grid, so every sum is
    exact in float32): two vertices at opposite corners in x and y, the third at the top in z."""
    sx, sy, sz = rng.choice([-1.0, 1.0], 3)
    p, q = rng.integers(-6, 7, 2) / 8.0
    off = np.array([[-sx, -sy, -sz], [sx, sy, -sz * rng.integers(0, 8) / 8.0], [p, q, sz]])
    return c + off * half


def box_centres(tris):
    """The BVH builder's centroid of a triangle: .5f * lo + .5f * hi of its bounding box, in float32."""
    t = np.asarray(tris, np.float32)
    return np.float32(0.5) * t.min(1) + np.float32(0.5) * t.max(1)


def coincident_centroids(seed=3, n_shards=1500):
    """Clusters of 6..20 triangles whose bounding-box centres are bit-identical (nested copies of one
    triangle scaled about the centre, so they lie in parallel planes and do not meet): the builder
    cannot split them and makes a leaf of more than 4 primitives. One more cluster's centres differ
    only in the last bit of x (half of it shifted by one ulp): a centroid range of one ulp for the
    SAH binning. Ordinary shards fill the space around them. sc.clusters: [(first triangle, count)]
    in the first mesh; sc.ulp_cluster: the same for the last-bit cluster."""
    rng = np.random.default_rng(seed)
    f = np.float32
    centres = np.array([[0.25, 0.5, 0.25], [0.75, 0.25, 0.5], [0.5, 0.75, 0.75], [0.75, 0.75, 0.25],
                        [0.25, 0.25, 0.75], [0.5, 0.375, 0.375]])
    sizes = [6, 9, 13, 17, 20, 12]
    tris, clusters = [], []
    for ci, (c, m) in enumerate(zip(centres, sizes)):
        half = np.array([0.125, 0.125, 0.125]) * rng.choice([0.5, 0.75, 1.0], 3)
        base = _centred_triangle(rng, np.zeros(3), half)
        shift = np.zeros(3)
        first = len(tris)
        for j in range(m):
            s = 1.0 - j / 32.0
            t = c + base * s
            if ci == len(sizes) - 1 and j % 2:  # the last-bit cluster: every other copy one ulp along x
                t = t + np.array([np.spacing(f(c[0])), 0.0, 0.0], np.float64)
            assert np.array_equal(t.astype(f).astype(np.float64), t), "cluster vertices must be exact in float32"
            tris.append(t)
        clusters.append((first, m))
    tris = np.asarray(tris)
    cen = box_centres(tris)
    for first, m in clusters[:-1]:
        assert len(np.unique(cen[first:first + m].view(np.uint32), axis=0)) == 1
    first, m = clusters[-1]
    xs = np.unique(cen[first:first + m, 0])
    assert len(xs) == 2 and xs[1] == xs[0] + np.spacing(xs[0])
    assert len(np.unique(cen[first:first + m, 1:].view(np.uint32), axis=0)) == 1
    keep = [(c, 0.23) for c in centres] + [([0.5, -0.9, 0.5], 0.06)]
    shards = _shards(rng, n_shards, [-0.2, -0.4, -0.2], [1.2, 1.2, 1.2], keep_out=keep, size=(2e-4, 0.2))
    light = ([0.3, -1.6, 2.6], 0.25)
    sc = _scene([_soup(tris), _soup(shards)], [0.5, -0.9, 0.5], [0.5, 0.5, 0.5], [0, 0, 1], 70.0, light,
                trace_eps=2e-5, min_dist=0.04)
    sc.clusters = clusters[:-1]
    sc.ulp_cluster = clusters[-1]
    return sc


def deep_tree(n, q=1.6, v0=256.0):
    """n triangles in six chains along +x, -x, +y, -y, +z, -z: triangle i is one base triangle (in the
    plane at distance 1, its bounding box centred on the axis) scaled by v_i = v0 q^-i about the origin
    and put on axis (i % 6) // 2, on the negative side for odd i. Its builder centroid is +-v_i on that
    axis and exactly 0 on the other two. At every level of the build the largest triangle left is
    alone at one end of the centroid range on its axis (the next one on the same side is q^6 > 16 times
    closer to 0, so it shares a bin with the bulk), and as everything else is smaller by then, peeling
    it off is the cheapest SAH split: the tree is a chain of depth n - 3 (measured with the product's
    builder, scene.cpp compiled for the host: 37 for n = 40, 47 -- the most the 48-entry traversal
    stack allows -- for n = 50, 48 for n = 51, 61 for n = 64). The sizes span q^n, 2^34 for n = 50,
    well inside what float32 products of three lengths can hold.

    The camera sits at the origin and looks along (1, 1, 1) as in shard_cloud: the +x, +y and +z chains
    are in frame, and from the origin every triangle of a chain covers the same directions, so a ray
    that meets one meets them all, at t growing by q^6 from one to the next (no ties), and walks the
    chain to its far end for the closest hit, the smallest triangle. The light is off the axes at
    the scale of the chains' middle: the origin and the small triangles around it see it, and the
    large triangles, which carry most of the sample points, lie mostly in the shadow of smaller ones."""
    base = np.array([[1.0, -0.5, -0.375], [1.0, 0.5, -0.125], [1.0, -0.125, 0.375]])
    tris = []
    for i in range(n):
        t = (base * float(np.float32(v0 * q ** -i))).astype(np.float32)
        if i % 2:
            t[:, 0] = -t[:, 0]
        tris.append(np.roll(t, (i % 6) // 2, axis=1))
    tris = np.stack(tris)
    cen = box_centres(tris)
    assert (cen != 0).sum(1).max() == 1 and np.all(np.diff(np.abs(cen).max(1)) < 0)
    light = ([0.6, 0.4, 0.5], 0.04)
    sc = _scene([_soup(tris)], [0, 0, 0], [1, 1, 1], [0.1, 0.25, 1.0], 150.0, light, trace_eps=0.0, min_dist=6.0)
    sc.rel_trace_eps = 1e-3  # shadow rays start this fraction of their triangle's size off it
    return sc
