"""The four BVH tracers on the GPU (bvh_trace.h: trace_closest, trace_closest_wave / _packet,
trace_any, trace_any_wave; replay_gen.hip's copies in test_replay_gpu.py) on the hostile
scenes of tests/synth.py, against the oracle's tracer -- itself pinned to a float64 brute force in
tests/test_trace_oracle.py -- and against that brute force.

  per-lane closest hit   mpss_tile_costs, one 1 x 1 rect per pixel: hit / miss equal to the oracle's on
                         every pixel, and to the brute force outside its too-close-to-call rays
  packet closest hit,    the 64 x 64 frame at 4 spp against the oracle's under tests/parity.py (weights
  wave any-hit           bit-equal, XYZ within 1e-4); four tiles meeting at an axis direction are
                         bit-identical to the full frame
  any-hit in Preprocess  surface points byte-equal, irradiance rtol 1e-5 and >= 99 % bit-identical, and
                         at least 5 % of the points lit and 5 % dark
  Poisson walk           per-lane closest hit over several bounces: the points equal the oracle's

  deep trees             deep_tree(40) and deep_tree(50) -- 47 levels, the most the 48-entry traversal
                         stack allows -- pass all of the above; deep_tree(51), 48 levels, and
                         deep_tree(64) are refused on the host, naming the traversal stack, before
                         anything is uploaded or launched (scene_upload.hip upload_scene). Accepting 50
                         and refusing 51 pins the depth of the chain to n - 3.

stacked_sheets: Preprocess starts a point's shadow rays minsampledistance / 10 off the surface, which
at a few thousand points is beyond the whole stack, so its dark points are those under the scene's
awning; sheet against sheet is what the render's and the oracle test's rays see.
coincident_centroids: that its clusters become leaves of more than 4 primitives (7 of them, up to
20, measured with scene.cpp compiled for the host) follows from scene.cpp's `chi[axis] <= clo[axis]`
leaf; no entry point exposes the leaf sizes to assert them here.
"""
import numpy as np
import pytest

import oracle_render as orr
import parity
import test_trace_oracle as tto

pytestmark = pytest.mark.gpu
RENDERED = tto.SCENES
SEED = 7


def _build(mpss, name, **cfg):
    from mpss import pbrtscene
    sc = tto.scene(name)
    ctx = pbrtscene.build_context(sc, **cfg)
    ctx.preprocess(seed=SEED)
    o = orr.OracleScene(sc, orr.tables_from_oracle(sc), ctx.cfg, mpss)
    return sc, ctx, o


@pytest.fixture(scope="module", params=tto.SCENES)
def traced(request, mpss, oracle):
    import torch
    assert torch.cuda.is_available()
    sc, ctx, o = _build(mpss, request.param)
    yield request.param, sc, ctx, o
    ctx.close()
    o.close()


@pytest.fixture(scope="module", params=RENDERED)
def rendered(request, mpss, oracle):
    import torch
    assert torch.cuda.is_available()
    sc, ctx, o = _build(mpss, request.param)
    yield request.param, sc, ctx, o
    ctx.close()
    o.close()


def test_per_lane_closest_hit(traced):
    name, sc, ctx, o = traced
    W, H = sc.xres, sc.yres
    _, surf = ctx.tile_costs([(x, x + 1, y, y + 1) for y in range(H) for x in range(W)])
    assert set(np.unique(surf)) <= {0, 1}
    got = surf.astype(bool)
    co, cd, ct, ctri, cany, cuns = tto.reference(name)["camera"]
    _, otri, _, _ = o.trace_closest(co, cd)
    bad = np.flatnonzero(got != (otri >= 0))
    assert len(bad) == 0, "%d pixels differ from the oracle, first (y, x) %s" % (
        len(bad), [(int(i) // W, int(i) % W) for i in bad[:5]])
    keep = ~cuns
    assert np.array_equal(got[keep], (ctri >= 0)[keep])
    assert 0.05 < got.mean() < 0.999
    img = got.reshape(H, W)
    for tw, th in ((W, 1), (8, 8), (13, 7)):  # whole rows (every wave full), tiles, ragged tiles
        rects = [(x, min(x + tw, W), y, min(y + th, H)) for y in range(0, H, th) for x in range(0, W, tw)]
        sss, surf = ctx.tile_costs(rects)
        assert [int(v) for v in surf] == [int(img[y0:y1, x0:x1].sum()) for x0, x1, y0, y1 in rects]
        assert np.array_equal(sss, surf)  # every surface here carries the BSSRDF, and the octree is built


def _render(ctx, sc, x0, x1, y0, y1, seed):
    import torch
    out = torch.zeros(((y1 - y0) * (x1 - x0) * 4,), dtype=torch.float32, device="cuda")
    ctx.render_tile(sc.spp, seed, x0, x1, y0, y1, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(y1 - y0, x1 - x0, 4)


def test_preprocess_any_hit(rendered):
    name, sc, ctx, o = rendered
    pts = ctx.surface_points()
    ref_pts = o.tessellate()
    assert 2000 <= len(pts) <= 8000
    assert len(pts) == len(ref_pts) and pts.tobytes() == ref_pts.tobytes()
    got = ctx.irradiance()
    ref = o.irradiance(pts, SEED)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6 * float(ref.max()))
    assert (got == ref).mean() >= 0.99
    lit = ref.max(1) > 0
    print("%s: %d points, %.1f %% lit, %.1f %% dark" % (name, len(pts), 100 * lit.mean(), 100 * (1 - lit.mean())))
    assert lit.mean() >= 0.05 and (~lit).mean() >= 0.05


def test_packet_closest_hit_and_wave_any_hit(rendered):
    name, sc, ctx, o = rendered
    pts = ctx.surface_points()
    o.set_octree(pts, o.irradiance(pts, SEED))
    W, H = sc.xres, sc.yres
    full = _render(ctx, sc, 0, W, 0, H, 5)
    ref = o.render_tile(sc.spp, 5, 0, W, 0, H)
    parity.check_image(full, ref, "trace_%s" % name)
    assert (ref[..., 1] > 0).mean() > 0.05
    # four tiles meeting at the pixel nearest the +z axis direction (where the x and y signs both flip)
    _, d = tto.reference(name)["camera"][:2]
    k = int(np.argmax(d[:, 2]))
    cx, cy = min(max(k % W, 8), W - 8), min(max(k // W, 8), H - 8)
    for x0, x1, y0, y1 in ((0, cx, 0, cy), (cx, W, 0, cy), (0, cx, cy, H), (cx, W, cy, H)):
        assert np.array_equal(_render(ctx, sc, x0, x1, y0, y1, 5), full[y0:y1, x0:x1]), (x0, x1, y0, y1)


def test_poisson_walk_on_shard_cloud(mpss, oracle):
    """FindPoissonPointDistribution's random walk (poisson_walk_kernel: per-lane trace_closest, several
    bounces per path) inside the shard cloud, as test_layeredskin_switches_gpu drives the finder."""
    from mpss import pbrtscene
    import copy
    sc = copy.copy(tto.scene("shard_cloud"))
    sc.integrator = dict(sc.integrator, usepoissonpointfinder="true", minsampledistance=0.05)
    ctx = pbrtscene.build_context(sc)
    o = None
    try:
        ctx.preprocess(seed=5)
        got = ctx.surface_points()
        o = orr.OracleScene(sc, orr.tables_from_oracle(sc), ctx.cfg, mpss)
        ref = o.poisson_points(5)
        assert len(got) == len(ref) and len(got) > 100
        assert np.array_equal(got["p"], ref["p"])
        for k in ("u", "v", "material", "area", "ray_eps"):
            assert np.array_equal(got[k], ref[k]), k
    finally:
        ctx.close()
        if o is not None:
            o.close()


@pytest.mark.parametrize("n", [51, 64])
def test_too_deep_a_tree_is_refused(mpss, n):
    """48 levels and more: refused by upload_scene on the host (build_bvh, bvh_depth, throw) before the
    tree is uploaded, so no kernel ever walks it."""
    from mpss import pbrtscene
    ctx = pbrtscene.build_context(tto.scene("deep_tree%d" % n))
    try:
        with pytest.raises(mpss.MpssError, match="traversal stack"):
            ctx.preprocess(seed=SEED)
    finally:
        ctx.close()
