"""Pixel filters on the GPU (hash sampler): film_filter_kernel and the halo that feeds whole extra pixels through the
camera pass, shading and the gather, against the numpy restatement tests/filter_ref.py and the CPU oracle.

scenes/skin.pbrt at 48 x 40 (the parity tests' small skin scene: minsampledistance 0.008, 128-entry tables).

  1 weights      W of every pixel = the restatement's sum of table weights over restated sample positions, the
                 out-of-frame ones included; |dW| <= n 2^-24 sum|w| (n float additions of the pixel's n weights)
  2 radiance     spp 1: the oracle's box film holds each in-frame sample's XYZ (pixels with W == 1); gaussian and
                 mitchell 2/2 films = the restated AddSample over those samples, on pixels >= R from the edge with
                 no other pixel within reach; |d| <= n 2^-24 sum|w x| + 1e-4 sum|w x| (the parity tests' per-sample
                 bound, |gpu - cpu| <= 1e-4 |cpu|, carried through the weights)
  3 slots        box 1.5/1.5 at spp 4 reaches exactly the 3 x 3 neighbourhood: the film = the 3 x 3 sum of the
                 oracle's default film, W equal, XYZ within the parity bound 1e-4 of the sums
  4 out of frame no geometry in view, one constant infinite light, mitchell 2/2: X/W, Y/W, Z/W are the light's
                 constant on every pixel, border rows and columns included
  5 tiling       one rectangle = 16 x 16 tiles = several batches, bit for bit
  6 default      set_pixel_filter(box, .5, .5) changes nothing, bit for bit
  7 refusal      the reference sampler refuses a non-default filter and renders again with the default
"""
import os

import numpy as np
import pytest

import filter_ref as fr
import oracle_render as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 40
SEED = 21       # test 2 and 3: the oracle's box film has W == spp on every pixel (asserted there)
EPS = 2.0 ** -24
PARITY = 1e-4   # tests/parity.py TOL
pytestmark = pytest.mark.gpu


def _load(pbrtscene, spp=4):
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "skin.pbrt"), xres=W, yres=H, spp=spp)
    sc.integrator["minsampledistance"] = 0.008
    for m in sc.materials:
        m["desired_length"] = 128
    return sc


def _render(torch, ctx, spp, seed, rects=None):
    """The frame as one rectangle (rects None) or assembled from rectangles rendered by one render_tiles call."""
    if rects is None:
        out = torch.zeros((H * W * 4,), dtype=torch.float32, device="cuda")
        ctx.render_tile(spp, seed, 0, W, 0, H, out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(H, W, 4)
    outs = [torch.zeros(((y1 - y0) * (x1 - x0) * 4,), dtype=torch.float32, device="cuda") for x0, x1, y0, y1 in rects]
    ctx.render_tiles(spp, seed, rects, [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    frame = np.full((H, W, 4), np.nan, np.float32)
    for (x0, x1, y0, y1), o in zip(rects, outs):
        frame[y0:y1, x0:x1] = o.cpu().numpy().reshape(y1 - y0, x1 - x0, 4)
    return frame


@pytest.fixture(scope="module")
def rig(mpss, oracle):
    """The context (no filter call made on it yet), its default-filter frames, and the oracle's films."""
    import torch
    assert torch.cuda.is_available()
    from mpss import pbrtscene
    sc = _load(pbrtscene)
    ctx = pbrtscene.build_context(sc)
    ctx.preprocess(seed=4)
    base = {spp: _render(torch, ctx, spp, SEED) for spp in (1, 4)}  # before any set_pixel_filter
    o = orr.OracleScene(sc, orr.tables_from_ctx(ctx, len(sc.materials)), ctx.cfg, mpss)
    pts = ctx.surface_points()
    o.set_octree(pts, o.irradiance(pts, 4))
    ref = {spp: o.render_tile(spp, SEED, 0, W, 0, H) for spp in (1, 4)}
    return torch, pbrtscene, sc, ctx, base, ref


CASES = [(k, None, None, {}) for k in fr.KINDS] + [("box", 1.5, 1.5, {}), ("gaussian", 1.5, 3.0, dict(alpha=1.0)),
                                                   ("mitchell", 3.0, 2.0, dict(B=0.0, C=0.5))]


def _describe(kind, xw, yw, params):
    ab = [params[n] for n in ("alpha", "B", "C", "tau") if n in params]
    return fr.describe(kind, xw, yw, *(ab + [None, None])[:2])


@pytest.mark.parametrize("kind,xw,yw,params", CASES, ids=["%s-%s" % (c[0], c[1] or "default") for c in CASES])
@pytest.mark.parametrize("spp", [4, 3])
def test_weights(rig, spp, kind, xw, yw, params):
    torch, _, sc, ctx, _, _ = rig
    f = _describe(kind, xw, yw, params)
    ctx.set_pixel_filter(kind, xw, yw, **params)
    got = _render(torch, ctx, spp, 33)[..., 3].astype(np.float64)
    _, _, X, Y = fr.image_positions(f, W, H, spp, 33)
    r = fr.add_samples(f, W, H, X, Y)
    err = np.abs(got - r["film"][..., 3])
    tol = r["n"] * EPS * r["absw"]
    print("%s spp %d: max |dW| %.3g, worst err / tol %.3g, n <= %d" % (kind, spp, err.max(), (err / tol).max(), r["n"].max()))
    assert r["n"].min() >= spp
    assert np.all(err <= tol)
    if kind in ("mitchell", "sinc"):
        assert r["absw"].max() > np.abs(r["film"][..., 3]).max()  # negative weights take part


@pytest.mark.parametrize("kind", ["gaussian", "mitchell"])
def test_radiance_against_oracle_samples(rig, kind):
    torch, _, sc, ctx, _, ref = rig
    f = fr.describe(kind)
    R = fr.halo(f[1])
    assert R == 3
    o1 = ref[1]
    bad = o1[..., 3] != 1  # an edge-rounded sample: the pixel's XYZ is not one sample's
    assert bad.mean() <= 0.01
    ctx.set_pixel_filter(kind)
    got = _render(torch, ctx, 1, SEED).astype(np.float64)
    px, py, X, Y = fr.image_positions(f, W, H, 1, SEED)
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    xyz = o1[py[inside], px[inside], :3]
    r = fr.add_samples(f, W, H, X[inside], Y[inside], xyz)
    # compared: >= R from the edge (no out-of-frame sample reaches them), and no bad pixel within reach
    keep = np.zeros((H, W), bool)
    keep[R:H - R, R:W - R] = True
    for y, x in zip(*np.nonzero(bad)):
        keep[max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1] = False
    assert keep.sum() >= 0.5 * W * H
    errw = np.abs(got[..., 3] - r["film"][..., 3])
    assert np.all(errw[keep] <= (r["n"] * EPS * r["absw"])[keep])
    err = np.abs(got[..., :3] - r["film"][..., :3])
    tol = r["n"][..., None] * EPS * r["absx"] + PARITY * r["absx"]
    print("%s: worst err / tol %.3g on %d pixels" % (kind, (err[keep] / np.maximum(tol[keep], 1e-300)).max(), keep.sum()))
    assert np.all(err[keep] <= tol[keep])
    assert (r["film"][keep][:, 1] > 0).mean() > 0.05  # the comparison covers shaded pixels


def test_slots_box_3x3_against_oracle(rig):
    torch, _, sc, ctx, _, ref = rig
    o4 = ref[4]
    assert np.all(o4[..., 3] == 4)  # no edge-rounded sample in the frame
    ctx.set_pixel_filter("box", 1.5, 1.5)
    got = _render(torch, ctx, 4, SEED)
    want = np.zeros((H, W, 4))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            want[1:H - 1, 1:W - 1] += o4[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx].astype(np.float64)
    g, w = got[2:H - 2, 2:W - 2].astype(np.float64), want[2:H - 2, 2:W - 2]
    assert np.array_equal(g[..., 3], w[..., 3]) and np.all(w[..., 3] == 36)
    assert np.array_equal(g[..., :3] == 0, w[..., :3] == 0)
    nz = w[..., :3] != 0
    rel = np.abs(g[..., :3] - w[..., :3])[nz] / np.abs(w[..., :3][nz])
    print("box 1.5: relative L-inf %.3g" % rel.max())
    assert rel.max() <= PARITY
    assert (w[..., 1] > 0).mean() > 0.05


def test_out_of_frame_samples_carry_radiance(mpss):
    import torch
    from mpss import pbrtscene
    from test_render_parity_gpu import _sky_light
    sc = _load(pbrtscene)
    sc.lights = [_sky_light(-70, [0, 1, 1], L=(0.2, 0.15, 0.12), scale=(1, 1, 1), ns=1)]
    sc.world_to_camera = np.diag([-1.0, 1.0, -1.0, 1.0]) @ sc.world_to_camera  # the camera turned round: nothing in view
    ctx = pbrtscene.build_context(sc)
    ctx.preprocess(seed=4)
    assert ctx.tile_costs([(0, W, 0, H)])[1][0] == 0
    base = _render(torch, ctx, 4, 5).astype(np.float64)
    assert np.all(base[..., 3] == 4)
    # every sample's XYZ is the light's constant, to the last bits of the 1 x 1 map's bilinear lookup
    c = np.median(base[..., :3].reshape(-1, 3), axis=0) / 4
    assert np.all(c > 0) and np.all(c <= 0.5) and np.all(np.abs(base[..., :3] / 4 - c) <= 4 * 2.0 ** -23 * c)
    f = fr.describe("mitchell")
    ctx.set_pixel_filter("mitchell")
    got = _render(torch, ctx, 4, 5).astype(np.float64)
    px, py, X, Y = fr.image_positions(f, W, H, 4, 5)
    r = fr.add_samples(f, W, H, X, Y)
    tolw = r["n"] * EPS * r["absw"]
    assert np.all(np.abs(got[..., 3] - r["film"][..., 3]) <= tolw)
    # test 1's tolerance over W (with c <= 0.5 that leaves room for X = sum w c and W both carrying the weights'
    # rounding: 2 c <= 1)
    ratio = got[..., :3] / got[..., 3:4]
    tol = (tolw / np.abs(got[..., 3]))[..., None] * np.ones(3)
    print("constant sky: worst |X/W - c| / tol %.3g" % (np.abs(ratio - c) / tol).max())
    assert np.all(np.abs(ratio - c) <= tol)
    # the border pixels do collect out-of-frame samples: more weight than the in-frame samples alone give
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    r_in = fr.add_samples(f, W, H, X[inside], Y[inside])
    assert np.all(r_in["n"][0, :] < r["n"][0, :]) and np.all(r_in["n"][:, W - 1] < r["n"][:, W - 1])


def test_tiling_and_batches_bit_equal(rig):
    torch, pbrtscene, sc, ctx, _, _ = rig
    ctx.set_pixel_filter("gaussian")
    whole = _render(torch, ctx, 4, 9)
    rects = [(x, min(x + 16, W), y, min(y + 16, H)) for y in range(0, H, 16) for x in range(0, W, 16)]
    tiled = _render(torch, ctx, 4, 9, rects)
    assert whole.tobytes() == tiled.tobytes()
    small = pbrtscene.build_context(sc, max_batch_samples=1 << 10)  # the frame in several batches
    small.preprocess(seed=4)
    small.set_pixel_filter("gaussian")
    small.set_instrumentation(kernel_timing=True)  # (counts the camera pass's launches: one per batch here)
    small.reset_render_stats()
    batched = _render(torch, small, 4, 9)
    assert small.render_stats()["n_camera"] >= 4
    assert whole.tobytes() == batched.tobytes()
    assert (whole[..., 1] > 0).mean() > 0.05


def test_default_filter_untouched(rig):
    torch, _, sc, ctx, base, ref = rig
    ctx.set_pixel_filter("gaussian")
    ctx.set_pixel_filter("box", 0.5, 0.5)
    for spp in (1, 4):
        assert _render(torch, ctx, spp, SEED).tobytes() == base[spp].tobytes()
    assert np.array_equal(base[4][..., 3], ref[4][..., 3])


def test_reference_sampler_refuses_other_filters(mpss):
    import torch
    from mpss import pbrtscene
    sc = _load(pbrtscene)
    ctx = pbrtscene.build_context(sc, sampler=mpss.SAMPLER_REFERENCE, replay_cores=8)
    ctx.preprocess(seed=0)
    before = _render(torch, ctx, 4, 0)
    ctx.set_pixel_filter("gaussian")
    out = torch.zeros((H * W * 4,), dtype=torch.float32, device="cuda")
    with pytest.raises(mpss.MpssError) as e:
        ctx.render_tile(4, 0, 0, W, 0, H, out.data_ptr())
    assert "error -1" in str(e.value) and "reference sampler" in str(e.value) and "filter" in str(e.value)
    with pytest.raises(mpss.MpssError):
        ctx.render_tiles(4, 0, [(0, 16, 0, 16)], [out.data_ptr()])
    ctx.set_pixel_filter("box")
    assert _render(torch, ctx, 4, 0).tobytes() == before.tobytes()


def test_abi_rejects_bad_filters_on_a_context(rig, mpss):
    _, _, _, ctx, _, _ = rig
    lib = mpss.lib()
    for args in ((7, 1.0, 1.0, 0.0, 0.0), (0, -0.5, 0.5, 0.0, 0.0), (2, 2.0, float("inf"), 2.0, 0.0),
                 (4, 4.0, 4.0, float("nan"), 0.0)):
        assert lib.mpss_set_pixel_filter(ctx.h, *args) == -1
        assert lib.mpss_last_error().decode().startswith("mpss_set_pixel_filter: ")
    assert lib.mpss_abi_version() == 13
