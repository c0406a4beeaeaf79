"""The spectral film (mpss_render_tile(s)_spectral) on the GPU: the 30-band radiance cube beside the XYZ film.

  1 the XYZW of a spectral call is mpss_render_tile's, bit for bit; the cube's slot 30 is its W, slot 31 is 0
  2 Spectrum::ToXYZ of the cube (mpss_host_spectrum_to_xyz) is the XYZ film up to the order of the float sums:
    every term is non-negative under the box and the gaussian, so per pixel and channel the two differ by at
    most (30 + S + 4) 2^-24 of the value, S the samples in the pixel's filter support (30 products and sums
    of ToXYZ, S weighted sums, the scale and the weight products); no floor, no value zero on one side only
  3 the cube does not depend on how the frame is cut into tiles, batches and pieces, bit for bit
  4 a light that emits in one band c only: the oracle's XYZ film then holds sum w L_c times ToXYZ(e_c), which
    pins band c of the cube to the oracle by tests/parity.py's criterion; every other band is exactly 0
  5 samples that the SamplerRenderer filter rejects (a NaN in the material's Rd table) leave 0 in every band
    and keep their weight
  6 bad arguments fail before anything is launched
  7 a pigment sweep writes cubes whose projection is the image it writes
"""
import os

import numpy as np
import pytest

import oracle_render as orr
import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 30
U = 2.0 ** -24


def _skin_scene(pbrtscene, res=64, spp=8):
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "skin.pbrt"), xres=res, yres=res, spp=spp)
    sc.integrator["minsampledistance"] = 0.008
    for m in sc.materials:
        m["desired_length"] = 128
    return sc


@pytest.fixture(scope="module")
def skin(mpss):
    import torch
    assert torch.cuda.is_available()
    from mpss import pbrtscene
    sc = _skin_scene(pbrtscene)
    ctx = pbrtscene.build_context(sc)
    ctx.preprocess(seed=11)
    yield torch, sc, ctx
    ctx.close()


def _xyzw(torch, ctx, spp, seed, x0, x1, y0, y1):
    out = torch.zeros(((y1 - y0) * (x1 - x0) * 4,), dtype=torch.float32, device="cuda")
    ctx.render_tile(spp, seed, x0, x1, y0, y1, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(y1 - y0, x1 - x0, 4)


def _spectral(torch, ctx, spp, seed, x0, x1, y0, y1, xyzw=True):
    """(cube rows [h, w, 32], XYZW [h, w, 4] or None) of one mpss_render_tile_spectral call; the buffers start
    as NaN, so every value read back was written."""
    n = (y1 - y0) * (x1 - x0)
    spec = torch.full((n * 32,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((n * 4,), float("nan"), dtype=torch.float32, device="cuda") if xyzw else None
    ctx.render_tile_spectral(spp, seed, x0, x1, y0, y1, spec.data_ptr(), out.data_ptr() if xyzw else None)
    torch.cuda.synchronize()
    return (spec.cpu().numpy().reshape(y1 - y0, x1 - x0, 32),
            out.cpu().numpy().reshape(y1 - y0, x1 - x0, 4) if xyzw else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_projection(mpss, spec, xyzw, S):
    """Test 2's criterion; returns the worst error in units of the bound."""
    proj = mpss.host_spectrum_to_xyz(spec[..., :NB]).astype(np.float64)
    ref = xyzw[..., :3].astype(np.float64)
    assert not np.isnan(proj).any() and not np.isnan(ref).any()
    assert np.all(ref >= 0) and ref.max() > 0
    assert int(((proj == 0) != (ref == 0)).sum()) == 0, "values zero on one side only"
    bound = (30 + S + 4) * U
    nz = ref != 0
    rel = np.abs(proj[nz] - ref[nz]) / ref[nz]
    worst = float(rel.max() / bound)
    print("projection: worst relative difference %.3g = %.3f of the bound %.3g (S = %d)" % (rel.max(), worst, bound, S))
    assert worst <= 1.0
    return worst


# ------------------------------------------------------------------ 1
@pytest.mark.gpu
@pytest.mark.parametrize("spp", [8, 4])
@pytest.mark.parametrize("rect", [(0, 64, 0, 64), (21, 45, 30, 57)])
def test_xyz_beside_the_cube_is_the_xyz_film(skin, spp, rect):
    """8 spp: film_kernel's 16-byte slot loads; 4 spp: its scalar tail. The ragged tile's borders cut through
    the face (edge samples of neighbours)."""
    torch, sc, ctx = skin
    ref = _xyzw(torch, ctx, spp, 5, *rect)
    spec, got = _spectral(torch, ctx, spp, 5, *rect)
    assert np.array_equal(_bits(got), _bits(ref))
    assert np.array_equal(_bits(spec[..., 30]), _bits(ref[..., 3]))
    assert np.array_equal(_bits(spec[..., 31]), np.zeros(spec.shape[:2], np.uint32))
    assert not np.isnan(spec).any() and (spec[..., :NB] > 0).any()
    alone, none = _spectral(torch, ctx, spp, 5, *rect, xyzw=False)  # the cube without an XYZW output
    assert none is None and np.array_equal(_bits(alone), _bits(spec))


# ------------------------------------------------------------------ 2
def _sky_scene(pbrtscene):
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "tissue_sky.pbrt"), xres=48, yres=48, spp=4)
    sc.integrator["minsampledistance"] = 0.008
    for m in sc.materials:
        m["desired_length"] = 128
    return sc


def _light_sphere_scene(pbrtscene):
    """test_render_parity_gpu's _visible_sphere_scene: a second sphere light in front of the face, in frame
    (camera rays that hit it return Le plus its matte surface's direct light), and a sky behind."""
    sc = _skin_scene(pbrtscene, res=48, spp=4)
    l2w = pbrtscene.rotate(40, [1, 1, 0])
    sky = dict(kind="infinite", L=[0.3, 0.35, 0.45], scale=[2, 2, 2], nsamples=2, l2w=l2w.astype(np.float32),
               w2l=np.linalg.inv(l2w).astype(np.float32))
    front = dict(center=[0.53, -2.53, 0.51], radius=0.12, L=[6.0, 5.0, 4.0], nsamples=2)
    sc.lights = [sc.lights[0], front, sky]
    return sc


@pytest.fixture(scope="module")
def scenes(mpss, skin):
    """name -> (scene, context): the skin frame of the other tests, a frame with escaped rays (the sky
    path) and one with a light sphere in view (Le)."""
    from mpss import pbrtscene
    made = {"skin": (skin[1], skin[2])}
    for name, make, seed in (("sky", _sky_scene, 6), ("sphere", _light_sphere_scene, 8)):
        sc = make(pbrtscene)
        ctx = pbrtscene.build_context(sc)
        ctx.preprocess(seed=seed)
        made[name] = (sc, ctx)
    yield made
    for name in ("sky", "sphere"):
        made[name][1].close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", ["box", "gaussian"])
@pytest.mark.parametrize("name", ["skin", "sky", "sphere"])
def test_projection_is_the_xyz_film(mpss, skin, scenes, name, filt):
    torch = skin[0]
    sc, ctx = scenes[name]
    S = 9 * sc.spp if filt == "box" else (2 * 2 + 1) ** 2 * sc.spp  # gaussian 2 / 2: ceil(r) = 2
    try:
        if filt != "box":
            ctx.set_pixel_filter(filt, 2.0, 2.0)
        spec, xyzw = _spectral(torch, ctx, sc.spp, 17, 0, sc.xres, 0, sc.yres)
    finally:
        ctx.set_pixel_filter("box")
    assert np.array_equal(_bits(spec[..., 30]), _bits(xyzw[..., 3]))
    assert np.array_equal(_bits(spec[..., 31]), np.zeros(spec.shape[:2], np.uint32))
    _check_projection(mpss, spec, xyzw, S)
    lit = (xyzw[..., 1] > 0).mean()
    assert lit > (0.5 if name != "skin" else 0.05)  # a sky fills the frame


@pytest.mark.gpu
def test_mitchell_weight_plane(skin):
    """Negative lobes: the bound of test 2 cannot be observed from the outputs; the weights and the tiling
    (below) still pin the kernel."""
    torch, sc, ctx = skin
    try:
        ctx.set_pixel_filter("mitchell")
        spec, xyzw = _spectral(torch, ctx, sc.spp, 17, 0, 64, 0, 64)
        ref = _xyzw(torch, ctx, sc.spp, 17, 0, 64, 0, 64)
        tiled = _tiled_cube(torch, ctx, sc.spp, 17, 64, 16)
    finally:
        ctx.set_pixel_filter("box")
    assert np.array_equal(_bits(xyzw), _bits(ref))
    assert np.array_equal(_bits(spec[..., 30]), _bits(ref[..., 3])) and (ref[..., 3] != 0).all()
    assert np.array_equal(_bits(tiled), _bits(spec))


# ------------------------------------------------------------------ 3
def _tiled_cube(torch, ctx, spp, seed, res, tile, xyzw=False):
    rects = [(x, x + tile, y, y + tile) for y in range(0, res, tile) for x in range(0, res, tile)]
    bufs = [torch.full((tile * tile * 32,), float("nan"), dtype=torch.float32, device="cuda") for _ in rects]
    # an XYZW output for every other rectangle only: the rest have none
    outs = [torch.zeros((tile * tile * 4,), dtype=torch.float32, device="cuda") if i % 2 == 0 else None
            for i in range(len(rects))] if xyzw else None
    ctx.render_tiles_spectral(spp, seed, rects, [b.data_ptr() for b in bufs],
                              None if outs is None else [None if o is None else o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    cube = np.zeros((res, res, 32), np.float32)
    for (x0, x1, y0, y1), b in zip(rects, bufs):
        cube[y0:y1, x0:x1] = b.cpu().numpy().reshape(tile, tile, 32)
    if not xyzw:
        return cube
    film = np.full((res, res, 4), np.nan, np.float32)
    for (x0, x1, y0, y1), o in zip(rects, outs):
        if o is not None:
            film[y0:y1, x0:x1] = o.cpu().numpy().reshape(tile, tile, 4)
    return cube, film


@pytest.mark.gpu
@pytest.mark.parametrize("filt", ["box", "gaussian"])
def test_cube_does_not_depend_on_tiling(mpss, skin, filt):
    """One 64 x 64 call; sixteen 16 x 16 tiles in one mpss_render_tiles_spectral call; and a context whose
    max_batch_samples (8192: 15 tile rows of the frame, three 16 x 16 tiles) cuts the frame into several
    pieces and batches, and packs several tiles' pieces into a batch."""
    from mpss import pbrtscene
    torch, sc, ctx = skin
    small = pbrtscene.build_context(sc, max_batch_samples=8192)
    try:
        small.preprocess(seed=11)
        if filt != "box":
            ctx.set_pixel_filter(filt, 2.0, 2.0)
            small.set_pixel_filter(filt, 2.0, 2.0)
        one, xyzw = _spectral(torch, ctx, sc.spp, 9, 0, 64, 0, 64)
        tiled, film = _tiled_cube(torch, ctx, sc.spp, 9, 64, 16, xyzw=True)
        cut, _ = _spectral(torch, small, sc.spp, 9, 0, 64, 0, 64)
        cut_tiled = _tiled_cube(torch, small, sc.spp, 9, 64, 16)
    finally:
        ctx.set_pixel_filter("box")
        small.close()
    assert (one[..., :NB] > 0).any() and not np.isnan(one).any()
    assert np.array_equal(_bits(tiled), _bits(one))
    assert np.array_equal(_bits(cut), _bits(one))
    assert np.array_equal(_bits(cut_tiled), _bits(one))
    have = ~np.isnan(film[..., 3])  # the rectangles that asked for XYZW have the frame's
    assert have.mean() == 0.5 and np.array_equal(_bits(film[have]), _bits(xyzw[have]))


# ------------------------------------------------------------------ 4
@pytest.mark.gpu
@pytest.mark.parametrize("band", [3, 15, 26])  # ToXYZ(e_c) is largest in Z, Y, X
def test_each_band_against_the_oracle(mpss, oracle, monkeypatch, band):
    import torch
    from mpss import pbrtscene
    sc = _skin_scene(pbrtscene)
    rgb = [float(v) for v in sc.lights[0]["L"]]
    plain = mpss.host_from_rgb
    emit = np.zeros(NB, np.float32)
    emit[band] = np.float32(plain(rgb).sum())  # the light's power, all of it in one band

    def one_band(v, illuminant=False):  # the light's Lemit on both sides; every other colour as it is
        return emit.copy() if [float(x) for x in v] == rgb else plain(v, illuminant)

    monkeypatch.setattr(mpss, "host_from_rgb", one_band)
    ctx = pbrtscene.build_context(sc)
    o = orr.OracleScene(sc, orr.tables_from_ctx(ctx, len(sc.materials)), ctx.cfg, mpss)
    monkeypatch.undo()
    try:
        ctx.preprocess(seed=11)
        pts = ctx.surface_points()
        E = o.irradiance(pts, 11)
        got_E = ctx.irradiance()
        np.testing.assert_allclose(got_E, E, rtol=1e-5, atol=1e-6 * float(E.max()))
        assert (E[:, band] > 0).any() and not np.delete(E, band, axis=1).any()
        o.set_octree(pts, E)
        spec, xyzw = _spectral(torch, ctx, sc.spp, 5, 0, sc.xres, 0, sc.yres)
        ref = o.render_tile(sc.spp, 5, 0, sc.xres, 0, sc.yres)
    finally:
        ctx.close()
        o.close()
    unit = np.zeros(NB, np.float32)
    unit[band] = 1
    coef = np.zeros(3, np.float32)
    oracle.lib().o_to_xyz(unit, coef)
    k = int(np.argmax(coef))
    assert k == {3: 2, 15: 1, 26: 0}[band]
    want = ref[..., k].astype(np.float64) / float(coef[k])  # sum of w L_c
    got = spec[..., band].astype(np.float64)
    # tests/parity.py's criterion on the one band: weights bit-exact, TOL relative L-inf, no floor, zero on
    # neither side alone
    assert np.array_equal(_bits(spec[..., 30]), _bits(ref[..., 3])), "film weights differ"
    assert int(((want == 0) != (got == 0)).sum()) == 0
    nz = want != 0
    rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    print("band %d: relative L-inf %.3g over %d lit pixels" % (band, rel.max(), nz.sum()))
    assert rel.max() <= parity.TOL
    assert nz.mean() > 0.05  # shaded skin is covered
    others = np.delete(spec[..., :NB], band, axis=2)
    assert np.array_equal(_bits(others), np.zeros(others.shape, np.uint32)), "a band without light is not +0"
    parity.check_image(xyzw, ref)  # and the XYZ film beside it is the oracle's


# ------------------------------------------------------------------ 5
def _tables_context(mpss, pbrtscene, sc, tab, rcp, rho):
    """The scene with its material installed from tables (mpss_set_material_tables)."""
    ctx = mpss.Context(**pbrtscene.integrator_config(sc))
    ctx.set_grid_builder(True)  # the host's per-knot scan of the common grids
    mid = ctx.set_material_tables(tab, rcp, rho)
    for me in sc.meshes:
        ctx.add_mesh(me["P"], me["indices"], me["o2w"], me["w2o"], mid, N=me["N"], S=me["S"], uv=me["uv"],
                     reverse=me["reverse"])
    for li in sc.lights:
        ctx.add_sphere_light(li["center"], li["radius"], mpss.host_from_rgb(li["L"]), li["nsamples"])
    r2c, c2w = sc.raster_to_camera()
    ctx.set_camera(r2c, c2w, sc.xres, sc.yres)
    ctx.preprocess(seed=11)
    return ctx


@pytest.mark.gpu
def test_rejected_samples_keep_their_weight(mpss, skin):
    """A run of NaN in one band's Rd table: a sample whose gather reads it has a NaN band, SamplerRenderer's
    filter zeroes the sample, and the pixel keeps the sum over its other samples in all 30 bands."""
    from mpss import pbrtscene
    torch, sc, ctx0 = skin
    tab, rcp, rho = ctx0.material_tables(0)[:3]
    bad = tab.copy()
    bad[12, 4000:4040] = np.nan  # a thin ring of distances: some gathers meet it, most do not
    frames = []
    for t in (tab, bad):
        ctx = _tables_context(mpss, pbrtscene, sc, t, rcp, rho)
        try:
            frames.append(_spectral(torch, ctx, sc.spp, 5, 0, 64, 0, 64))
        finally:
            ctx.close()
    (clean, clean_xyzw), (spec, xyzw) = frames
    assert not np.isnan(spec).any() and not np.isnan(xyzw).any()
    assert np.array_equal(_bits(spec[..., 30]), _bits(clean[..., 30]))  # the weights do not know
    assert np.array_equal(_bits(spec[..., 30]), _bits(xyzw[..., 3]))
    changed = (xyzw[..., :3] != clean_xyzw[..., :3]).any(axis=2)
    print("rejected samples: %d of %d lit pixels changed" % (changed.sum(), (clean_xyzw[..., 1] > 0).sum()))
    assert changed.any(), "no sample met the NaN entries"
    # a pixel that lost samples holds less in every band (L >= 0), and some pixels are untouched
    assert np.all(spec[..., :NB][changed] <= clean[..., :NB][changed])
    assert (xyzw[..., 1] > 0).any() and (~changed & (xyzw[..., 1] > 0)).any()
    _check_projection(mpss, spec, xyzw, 9 * sc.spp)


# ------------------------------------------------------------------ the reference sampler
@pytest.mark.gpu
def test_reference_sampler(mpss):
    """MPSS_SAMPLER_REFERENCE (pbrt's own task streams, replayed per window): the films read the same
    flags and slots whatever drew the samples, so the XYZW beside the cube and the W plane are render_tile's
    bit for bit, on a full frame and on the ragged tile, and the projection holds; another pixel filter is
    refused as for render_tile."""
    import torch
    from mpss import pbrtscene
    sc = _skin_scene(pbrtscene)
    ctx = pbrtscene.build_context(sc, sampler=mpss.SAMPLER_REFERENCE, replay_cores=8)
    try:
        ctx.preprocess(seed=11)
        for rect in ((21, 45, 30, 57), (0, 64, 0, 64)):
            ref = _xyzw(torch, ctx, sc.spp, 5, *rect)
            spec, got = _spectral(torch, ctx, sc.spp, 5, *rect)
            assert np.array_equal(_bits(got), _bits(ref))
            assert np.array_equal(_bits(spec[..., 30]), _bits(ref[..., 3]))
            assert np.array_equal(_bits(spec[..., 31]), np.zeros(spec.shape[:2], np.uint32))
            _check_projection(mpss, spec, got, 9 * sc.spp)
        assert (ref[..., 1] > 0).mean() > 0.05
        ctx.set_pixel_filter("gaussian")
        buf = torch.zeros((8 * 8 * 32,), dtype=torch.float32, device="cuda")
        with pytest.raises(mpss.MpssError, match="default pixel filter"):
            ctx.render_tile_spectral(sc.spp, 5, 0, 8, 0, 8, buf.data_ptr())
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6
@pytest.mark.gpu
def test_bad_arguments_fail_before_any_launch(mpss, skin):
    torch, sc, ctx = skin
    ctx.reset_render_stats()
    buf = torch.zeros((64 * 64 * 32,), dtype=torch.float32, device="cuda")
    with pytest.raises(mpss.MpssError, match="null"):
        ctx.render_tile_spectral(sc.spp, 1, 0, 8, 0, 8, None, buf.data_ptr())
    with pytest.raises(mpss.MpssError, match="null"):
        ctx.render_tiles_spectral(sc.spp, 1, [(0, 8, 0, 8), (8, 16, 0, 8)], [buf.data_ptr(), None])
    for rect in ((8, 8, 0, 8), (0, 8, 9, 3), (0, 65, 0, 8)):  # empty, inverted, outside: as render_tile
        with pytest.raises(mpss.MpssError, match="rectangle"):
            ctx.render_tile(sc.spp, 1, *rect, buf.data_ptr())
        with pytest.raises(mpss.MpssError, match="rectangle"):
            ctx.render_tile_spectral(sc.spp, 1, *rect, buf.data_ptr(), None)
    ctx.render_tiles_spectral(sc.spp, 1, [], [])  # no rectangles: nothing to do, as render_tiles
    torch.cuda.synchronize()
    assert ctx.render_stats()["samples"] == 0 and not buf.any().item()


# ------------------------------------------------------------------ 7
@pytest.mark.gpu
def test_sweep_writes_cubes(mpss, tmp_path):
    """Two rows of the pigment csv at 32 x 32: the cube file's projection (ToXYZ, XYZToRGB, the clamp) is
    the image file, within the half rounding of the image's channels."""
    from mpss import film, imageio, pbrtscene
    from mpss import sweep as sw
    rows = sw.read_rows(os.path.join(ROOT, "tests", "golden", "perms_first16.csv"), 2)
    sc = _skin_scene(pbrtscene, res=32, spp=4)
    n = 0
    for i, ((xyzw, spec), secs, ctx) in enumerate(sw.sweep(sc, rows, spectral=True)):
        assert xyzw.shape == (32, 32, 4) and spec.shape == (32, 32, 32)
        img, cube = str(tmp_path / ("perm_%d.exr" % i)), str(tmp_path / ("perm_%d_spectral.exr" % i))
        film.write_image(img, film.finalize(xyzw))
        film.write_spectral_exr(cube, film.finalize_spectral(spec))
        planes = imageio.read_exr_channels(cube)
        assert list(planes) == film.spectral_channel_names()
        bands = np.stack([planes[nm] for nm in planes], -1)
        assert np.array_equal(_bits(bands), _bits(film.finalize_spectral(spec)))
        xyz = mpss.host_spectrum_to_xyz(bands)
        rgb = np.maximum(np.float32(0), film.xyz_to_rgb(xyz)).astype(np.float64)
        ref = imageio.read_exr(img).astype(np.float64)
        # half: 2^-11 relative (2^-25 below its normal range); the float sums before it: the bound of test 2
        # and the weight division, through XYZToRGB's rows (absolute sum <= 5.3)
        slack = 5.3 * (30 + 9 * sc.spp + 8) * U * np.abs(xyz).max(axis=2, keepdims=True).astype(np.float64)
        assert np.all(np.abs(rgb - ref) <= 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + slack)
        assert (ref > 0).mean() > 0.05
        n += 1
    assert n == 2
