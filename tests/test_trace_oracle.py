"""The oracle's ray tracer (oracle/render.c intersect / occluded, exported as o_trace_closest /
o_trace_any) against a float64 brute force over every triangle, on the hostile scenes of
tests/synth.py. CPU only: this pins the checker's geometry to something other than itself; the GPU
tracers are then held to the checker (and to this brute force) in tests/test_trace_gpu.py.

Per scene: the 64 x 64 pixel-centre rays (closest hit) and 4096 shadow rays from triangle centroids,
started a little off the triangle on the light's side, to points on the light (any hit; and which
triangle a closest-hit walk of the same segment finds).

  hit / miss, triangle id     equal (camera rays; shadow segments too)
  t                           within 1e-5 relative, on the camera rays and the shadow segments, for
                              every camera hit, and every shadow hit whose float32 forward error
                              bound allows it (_t_resolvable; the other hits' measured error, up to
                              2e-4 for a blocker 1e-4 away, is printed)
  any-hit                     equal (shadow segments)

A ray is left out only when the float64 reference itself is within rounding of two answers: some
triangle in front of it has a barycentric coordinate within 1e-5 of an edge it passes (the other two
inside [-1e-5, 1 + 1e-5]), or its two closest hits differ in t by less than 1e-6 relative. At most 2 %
of a scene's rays may be left out (asserted); measured: 0 % shard_cloud, 0.05 % stacked_sheets,
0.51 % coincident_centroids (nested similar triangles share edge directions), 0.01 % deep_tree(40)
and deep_tree(50).
"""
import functools

import numpy as np
import pytest

import oracle_render as orr
import synth

SCENES = ["shard_cloud", "stacked_sheets", "coincident_centroids", "deep_tree40", "deep_tree50"]
N_SHADOW = 4096
EDGE = 1e-5      # barycentric distance to an edge below which a ray may be left out
TIE = 1e-6       # relative t distance of the two closest hits below which a ray may be left out
MAX_EXCLUDED = 0.02


@functools.lru_cache(maxsize=None)
def scene(name):
    return synth.deep_tree(int(name[9:])) if name.startswith("deep_tree") else getattr(synth, name)()


def shadow_rays(sc, n=N_SHADOW, seed=77):
    """n segments from triangle centroids, started sc.trace_eps (or sc.rel_trace_eps of the triangle's
    longest edge) off the triangle along +-normal, to points on the near side of the light's sphere:
    o, d = target - o (not normalised), mint = 0, maxt = 0.999, and the triangle each starts on."""
    rng = np.random.default_rng(seed)
    T = synth.scene_triangles(sc).astype(np.float64)
    tri = rng.integers(0, len(T), n)
    t = T[tri]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    eps = np.full(n, sc.trace_eps)
    if getattr(sc, "rel_trace_eps", None):
        eps = sc.rel_trace_eps * np.linalg.norm(t[:, 1] - t[:, 0], axis=1)
    c, r = np.asarray(sc.lights[0]["center"], np.float64), sc.lights[0]["radius"]
    side = np.where(((c - t.mean(1)) * nrm).sum(1) < 0, -1.0, 1.0)  # the side the light is on: no self-hit
    o = (t.mean(1) + nrm * (side * eps)[:, None]).astype(np.float32)
    w = c - o
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    xi = rng.standard_normal((n, 3))
    xi *= (rng.random(n) ** (1 / 3) / np.linalg.norm(xi, axis=1))[:, None]
    u = -w + 0.8 * xi                       # a direction within ~53 degrees of the one facing the origin
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = (c + r * u - o).astype(np.float32)
    return o, d, np.zeros(n, np.float32), np.full(n, 0.999, np.float32), tri, side


class Brute:
    """Moller-Trumbore in float64 over all triangles, no acceleration structure. The triangles are the
    ones both tracers hold: p1 and the float32 edges p2 - p1, p3 - p1."""

    def __init__(self, sc):
        T = synth.scene_triangles(sc)
        self.p1 = T[:, 0].astype(np.float64)
        self.e1 = (T[:, 1] - T[:, 0]).astype(np.float64)   # float32 differences, as the tracers store them
        self.e2 = (T[:, 2] - T[:, 0]).astype(np.float64)
        self.c = np.asarray(sc.lights[0]["center"], np.float32).astype(np.float64)
        self.r = float(np.float32(sc.lights[0]["radius"]))

    def _sphere(self, o, d, mint, maxt):
        """Nearest root of the light's sphere inside [mint, maxt], inf if none."""
        ro = o - self.c
        A, B, C = (d * d).sum(1), 2 * (d * ro).sum(1), (ro * ro).sum(1) - self.r ** 2
        disc = B * B - 4 * A * C
        ok = disc >= 0
        rd = np.sqrt(np.where(ok, disc, 0))
        t0, t1 = (-B - rd) / (2 * A), (-B + rd) / (2 * A)
        t = np.where((t0 >= mint) & (t0 <= maxt), t0, np.where((t1 >= mint) & (t1 <= maxt), t1, np.inf))
        return np.where(ok, t, np.inf)

    def trace(self, o, d, mint, maxt, chunk=256):
        """Per ray: closest t, its triangle (-1 the light's sphere, NO_HIT a miss), any-hit, and whether
        the reference is too close to call (see the module docstring)."""
        d = np.asarray(d, np.float64).reshape(-1, 3)
        n = len(d)
        o = np.broadcast_to(np.asarray(o, np.float64), d.shape)
        mint = np.broadcast_to(np.asarray(mint, np.float64), n)
        maxt = np.broadcast_to(np.asarray(maxt, np.float64), n)
        tt, tri = np.full(n, np.inf), np.full(n, orr.NO_HIT, np.int64)
        anyhit, unsure = np.zeros(n, bool), np.zeros(n, bool)
        for a in range(0, n, chunk):
            s = slice(a, min(n, a + chunk))
            O, D = o[s, None, :], d[s, None, :]
            lo, hi = mint[s, None], maxt[s, None]
            s1 = np.cross(D, self.e2[None])
            div = (s1 * self.e1[None]).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / div
                dd = O - self.p1[None]
                b1 = (dd * s1).sum(-1) * inv
                s2 = np.cross(dd, self.e1[None])
                b2 = (D * s2).sum(-1) * inv
                t = (self.e2[None] * s2).sum(-1) * inv
            b0 = 1.0 - b1 - b2
            ok = (div != 0) & (b1 >= 0) & (b2 >= 0) & (b0 >= 0) & (t >= lo) & (t <= hi)
            th = np.where(ok, t, np.inf)
            k = th.argmin(1)
            best = th[np.arange(len(k)), k]
            th[np.arange(len(k)), k] = np.inf
            second = th.min(1)
            ts = self._sphere(o[s], d[s], mint[s], maxt[s])
            anyhit[s] = np.isfinite(best) | np.isfinite(ts)
            tri[s] = np.where(np.isfinite(best), k, orr.NO_HIT)
            tri[s] = np.where(ts < best, -1, tri[s])
            tt[s] = np.minimum(best, ts)
            # too close to call: an edge within EDGE of the ray on a triangle in front of it ...
            bmin = np.minimum(np.minimum(b1, b2), b0)
            bmax = np.maximum(np.maximum(b1, b2), b0)
            near = (div != 0) & (t > 0) & (t <= hi * (1 + 1e-5)) & (np.abs(bmin) < EDGE) & (bmax < 1 + EDGE) & \
                (b1 + b2 + b0 - bmin - bmax > -EDGE)
            unsure[s] = near.any(1)
            # ... or the two closest hits within TIE of each other
            two = np.sort(np.stack([best, second, ts], 1), 1)[:, :2]
            with np.errstate(invalid="ignore"):
                unsure[s] |= np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] < TIE * two[:, 1])
        return tt, tri, anyhit, unsure


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scene's rays and the brute force's answers, computed once per session and shared with
    tests/test_trace_gpu.py: dict(camera=(o, d, t, tri, any, unsure), shadow=(o, d, mint, maxt, from_tri,
    side, t, tri, any, unsure))."""
    sc = scene(name)
    br = Brute(sc)
    o, d = synth.pixel_centre_rays(sc)
    cam = (o, d) + br.trace(o, d, 0.0, np.inf)
    so, sd, lo, hi, ftri, side = shadow_rays(sc)
    sh = (so, sd, lo, hi, ftri, side) + br.trace(so, sd, lo, hi)
    for a in cam + sh:
        a.setflags(write=False)
    return dict(camera=cam, shadow=sh)


def oracle_scene(sc):
    import mpss
    from mpss import pbrtscene
    tables = [(np.zeros((orr.NB, 2), np.float32), np.ones(orr.NB, np.float32), np.zeros(2, np.float32))] * len(
        sc.materials)  # the tracer reads no material table
    return orr.OracleScene(sc, tables, mpss.default_config(**pbrtscene.integrator_config(sc)), mpss)


def _t_resolvable(sc, o, d, ref_t, ref_tri):
    """Whether float32 can give a hit's t to 1e-5 relative at all: a forward error bound of
    Moller-Trumbore's t = (e2 . s2) / (s1 . e1), s1 = d x e2, s2 = (o - p1) x e1, with u = 2^-24 per
    rounded operation (the differences and cross products round once per component, a 3-term dot
    product three times), evaluated in float64 on the reference's hit triangle:
      |dN| <= u (3 sum |e2_k s2_k| + 2 |e2| |o - p1| |e1|),  |dD| <= u (3 sum |s1_k e1_k| + |e1| |d| |e2|),
      |dt| / t <= |dN| / |N| + |dD| / |D| + 2 u.
    It passes 1e-5 for a blocker much nearer than its triangle is large, for slivers and at grazing
    angles; such hits are compared by triangle id only."""
    T = synth.scene_triangles(sc)
    hit = ref_tri >= 0
    k = np.where(hit, ref_tri, 0)
    p1 = T[k, 0].astype(np.float64)
    e1, e2 = (T[k, 1] - T[k, 0]).astype(np.float64), (T[k, 2] - T[k, 0]).astype(np.float64)
    d = np.asarray(d, np.float64)
    dd = np.broadcast_to(np.asarray(o, np.float64), p1.shape) - p1
    s1, s2 = np.cross(d, e2), np.cross(dd, e1)
    ln = lambda v: np.linalg.norm(v, axis=1)
    u = 2.0 ** -24
    dN = u * (3 * np.abs(e2 * s2).sum(1) + 2 * ln(e2) * ln(dd) * ln(e1))
    dD = u * (3 * np.abs(s1 * e1).sum(1) + ln(e1) * ln(d) * ln(e2))
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = dN / np.abs((e2 * s2).sum(1)) + dD / np.abs((s1 * e1).sum(1)) + 2 * u
    return ~hit | (bound <= 1e-5)


def _compare(name, kind, got_t, got_tri, got_any, ref_t, ref_tri, ref_any, unsure, resolvable=None):
    keep = ~unsure
    share = unsure.mean()
    print("%s %s: %d rays, %.3f %% left out, %d hit a triangle, %d miss" % (
        name, kind, len(unsure), 100 * share, (ref_tri >= 0).sum(), (ref_tri == orr.NO_HIT).sum()))
    bad = np.flatnonzero(keep & (got_tri != ref_tri))
    assert len(bad) == 0, "%s %s: %d rays differ in hit or triangle, first %s (oracle %s, float64 %s)" % (
        name, kind, len(bad), bad[:5].tolist(), got_tri[bad[:5]].tolist(), ref_tri[bad[:5]].tolist())
    hit = keep & (ref_tri != orr.NO_HIT)
    rel = np.abs(got_t.astype(np.float64) - np.where(hit, ref_t, 1)) / np.where(hit, ref_t, 1)
    near = hit & ~resolvable
    hit &= resolvable
    print("%s %s: t of %d hits off by at most %.3g relative; %d more hits too near their origin for float32, off "
          "by at most %.3g" % (name, kind, hit.sum(), rel[hit].max() if hit.any() else 0, near.sum(),
                               rel[near].max() if near.any() else 0))
    assert not hit.any() or rel[hit].max() <= 1e-5, "%s %s: t off by %g relative" % (name, kind, rel[hit].max())
    if got_any is not None:
        bad = np.flatnonzero(keep & (got_any != ref_any))
        assert len(bad) == 0, "%s %s: %d any-hit answers differ, first %s" % (name, kind, len(bad), bad[:5].tolist())
    return share


@pytest.mark.parametrize("name", SCENES)
def test_oracle_tracer_matches_float64_brute_force(oracle, name):
    sc = scene(name)
    ref = reference(name)
    o = oracle_scene(sc)
    co, cd, ct, ctri, cany, cuns = ref["camera"]
    t, tri, _, _ = o.trace_closest(co, cd)
    _compare(name, "camera", t, tri.astype(np.int64), None, ct, ctri, cany, cuns, np.ones(len(ct), bool))  # all held
    so, sd, lo, hi, ftri, side, st, stri, sany, suns = ref["shadow"]
    t, tri, _, _ = o.trace_closest(so, sd, lo, hi)
    got_any = o.trace_any(so, sd, lo, hi)
    _compare(name, "shadow", t, tri.astype(np.int64), got_any, st, stri, sany, suns, _t_resolvable(sc, so, sd, st, stri))
    assert np.array_equal(got_any, tri != orr.NO_HIT)  # the oracle's two walks agree with each other
    excluded = (cuns.sum() + suns.sum()) / float(len(cuns) + len(suns))
    print("%s: %.3f %% of all rays left out" % (name, 100 * excluded))
    assert excluded <= MAX_EXCLUDED
    # the scene is not an easy one: camera rays both hit and miss, shadow rays are both free and blocked
    assert 0.1 < (ctri >= 0).mean() < 0.999 or name == "stacked_sheets"
    assert 0.05 < sany.mean() < 0.995
    o.close()


def test_shard_cloud_is_hostile():
    sc = scene("shard_cloud")
    o, d = synth.pixel_centre_rays(sc)
    assert np.all(d != 0)
    assert len(np.unique(synth.sign_octants(d))) >= 7
    per_wave = synth.wave_octant_counts(sc, d)
    assert per_wave.max() >= 3 and (per_wave >= 2).sum() >= 20
    T = synth.scene_triangles(sc)
    assert 2900 <= len(T) <= 4096
    aspect, ln = synth.triangle_aspects(T)
    assert ln.max() / ln.max(1).min() >= 500          # longest edges over ~three decades
    assert 0.07 <= (aspect >= 1e3).mean() <= 0.13     # about 10 % slivers
    # the camera is inside the cloud's box
    assert np.all(T.reshape(-1, 3).min(0) < o) and np.all(o < T.reshape(-1, 3).max(0))


def test_stacked_sheets_front_sheet_wins(oracle):
    """Closest hit is always the front sheet (mesh 0); a shadow ray that starts on a back sheet (a quarter
    of the gap off it, toward the light) is blocked."""
    sc = scene("stacked_sheets")
    ref = reference("stacked_sheets")
    o = oracle_scene(sc)
    co, cd, ct, ctri, cany, cuns = ref["camera"]
    hit = ctri >= 0
    front = hit & (ctri < sc.sheet_tris)
    assert front.mean() > 0.3 and np.all(front | (ctri >= sc.n_sheet_tris) | ~hit)  # sheet 0, or the awning
    t, tri, _, _ = o.trace_closest(co, cd)
    assert np.array_equal(tri >= 0, hit) and np.array_equal(tri[hit] < sc.sheet_tris, front[hit])
    so, sd, lo, hi, ftri, side, st, stri, sany, suns = ref["shadow"]
    back = (ftri >= sc.sheet_tris) & (ftri < sc.n_sheet_tris)
    assert back.sum() > 3000 and np.all(sany[back]) and np.all(o.trace_any(so, sd, lo, hi)[back])
    # neighbouring sheets are 1e-4 of the scene's size apart and parallel
    h = [np.asarray(m["P"], np.float64) @ sc.sheet_normal for m in sc.meshes[:8]]
    size = np.ptp(np.asarray(sc.meshes[0]["P"], np.float64), axis=0).max()
    mean = np.array([x.mean() for x in h])
    gaps = mean[:-1] - mean[1:]
    assert np.all(np.abs(gaps / size - 1e-4) < 2e-6) and max(np.ptp(x) for x in h) < 1e-6
    # seen at about 30 degrees from the sheet plane
    view = -co / np.linalg.norm(co)
    assert abs(np.degrees(np.arcsin(abs(view @ sc.sheet_normal))) - 30) < 1
    o.close()


def test_coincident_centroids_clusters():
    sc = scene("coincident_centroids")
    T = synth.scene_triangles(sc)
    cen = synth.box_centres(T)
    for first, m in sc.clusters:
        assert 6 <= m <= 20
        assert len(np.unique(cen[first:first + m].view(np.uint32), axis=0)) == 1
    first, m = sc.ulp_cluster
    x = cen[first:first + m, 0].view(np.uint32).astype(np.int64)
    assert np.ptp(x) == 1 and not np.ptp(cen[first:first + m, 1:], axis=0).any()
    assert len(T) > 1000  # ordinary shards around them


def test_deep_tree_centroids():
    """What makes the builder peel one triangle per level (synth.deep_tree): one nonzero centroid
    coordinate each, its size falling by 1.6 a step, the axis and the side taking turns."""
    for n in (40, 50, 51, 64):
        cen = synth.box_centres(synth.scene_triangles(synth.deep_tree(n))).astype(np.float64)
        k = np.arange(n)
        assert np.array_equal(np.abs(cen).argmax(1), (k % 6) // 2) and np.all((cen != 0).sum(1) == 1)
        v = cen[k, (k % 6) // 2]
        assert np.array_equal(np.sign(v), np.where(k % 2, -1.0, 1.0))
        assert np.allclose(np.abs(v), 256.0 * 1.6 ** -k, rtol=1e-6)
        assert np.all(np.abs(v[:-6]) > 16 * np.abs(v[6:]))  # the next one on the same side: in the bulk's bin
