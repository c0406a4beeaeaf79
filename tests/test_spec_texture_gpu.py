"""LayeredSkin "texture Kr" / "texture Kt" on the GPU: the hit's R, T and lobe set from its own lookups
(shade_tex_spec_kernel, shade_direct_spec_kernel, direct_combine_spec_kernel; shade_tex_filter_spec_kernel
under a pixel filter).

The oracle has no Kr / Kt texture but takes a constant R and T per material, so parity is checked on a
texture that is constant per surface:

  1 blocks    four planar quads facing the camera, one material each, one 64 x 16 texture of four 16 x 16 blocks
              (a bright grey, a saturated colour, exactly black, a dim colour; powers of two, so no resampling
              and box-filtered levels 0-4 stay pure per block). Quad k's uv rectangle lies in the middle of
              block k, so every lookup returns block k's colour (asserted on the host, 4 ulp per channel) and
              the oracle renders quad k with the constant R = FromRGB(colour k). Kr textured (Kt black: the
              black block takes ncomp 1 -> 0), Kt textured (Kr constant: 2 -> 1), both (Kt's blocks rotated by
              one: R black with T not, T black with R not), and Kt textured with the light behind the quads
              (the transmission lobe's value reaches the image). _check of test_render_parity_gpu.py: weights
              bit-exact, XYZ within 1e-4 relative.
  2 halo      the "both" scene under PixelFilter "gaussian" at spp 1 against the oracle's samples, as
              test_pixel_filter_gpu.py's test 2
  3 constant  scenes/skin.pbrt (albedo and bump textures on) with a Kr texture whose texels all equal c against
              "color Kr" c: relative 1e-5 per value, floor 1e-6 of the peak (a filtered lookup of equal texels is
              the texel times a weight sum that is 1 within a few roundings, <= 1e-6; the rest of the pipeline
              is the same; 10 x margin); c = 0 bit for bit
  4 ABI       the entry point by symbol, ABI version 13, its refusals, bindings kept by update_layeredskin and
              by set_material_textures, n_tex
"""
import os

import numpy as np
import pytest

import filter_ref as fr
import oracle_render as orr
from test_render_parity_gpu import _check, _render_gpu
from test_texture_gpu import ALBEDO, BUMP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 48
Z, HALF, OFF = 3.0, 0.6, 0.8  # the quads: squares of half-width HALF centred at (+-OFF, +-OFF, Z)
COLOURS = [(0.8, 0.8, 0.8), (1.0, 0.1, 0.3), (0.0, 0.0, 0.0), (0.05, 0.04, 0.03)]
EPS = 2.0 ** -24


def _blocks(colours):
    t = np.zeros((16, 64, 3), np.float32)
    for k, c in enumerate(colours):
        t[:, 16 * k:16 * k + 16] = c
    return dict(texels=t, wrap="clamp")  # gamma 1, scale 1, EWA


TEX = _blocks(COLOURS)
TEX_ROT = _blocks(COLOURS[1:] + COLOURS[:1])  # block k holds colour k + 1
GREY = [0.6, 0.6, 0.6]


def _uv_rect(k):
    """Quad k's uv rectangle: the middle eighth of block k in u, the middle quarter in v."""
    return k / 4 + 3 / 32, k / 4 + 5 / 32, 3 / 8, 5 / 8


def _quad_scene(pbrtscene, materials, spp=4, back_light=False):
    sc = pbrtscene.Scene()
    sc.xres, sc.yres, sc.spp, sc.fov = W, H, spp, 60.0
    # (91 k points: coarser ones leave Mo() spikes next to them that dwarf the specular term test 1 looks for)
    sc.integrator = dict(maxdepth=5, maxerror=0.1, minsampledistance=0.0125)
    sc.materials = materials
    eye = np.eye(4, dtype=np.float32)
    for k, (sx, sy) in enumerate([(-1, -1), (1, -1), (-1, 1), (1, 1)]):
        cx, cy = sx * OFF, sy * OFF
        P = np.array([[cx - HALF, cy - HALF, Z], [cx + HALF, cy - HALF, Z], [cx + HALF, cy + HALF, Z],
                      [cx - HALF, cy + HALF, Z]], np.float32)
        u0, u1, v0, v1 = _uv_rect(k)
        # v runs against y: cross(dpdu, dpdv), the surface normal, points at the camera and the light
        uv = np.array([[u0, v1], [u1, v1], [u1, v0], [u0, v0]], np.float32)
        sc.meshes.append(dict(P=P, N=None, S=None, uv=uv, indices=np.array([[0, 1, 2], [0, 2, 3]], np.int32),
                              o2w=eye, w2o=eye, reverse=False, material=k))
    sc.lights = [dict(center=[0.0, 0.0, 7.0 if back_light else -1.0], radius=0.3, L=[40.0, 40.0, 40.0], nsamples=4)]
    return sc


def _case(which):
    """(the product's material dicts, the oracle's) of a case: quad k textured / constant at block k's colour."""
    prod, orc = [], []
    for k in range(4):
        base = dict(desired_length=128)
        if which in ("kr", "white"):
            prod.append(dict(base, Kt=[0.0] * 3, **(dict(kr_tex=TEX) if which == "kr" else dict(Kr=[1.0] * 3))))
            orc.append(dict(base, Kt=[0.0] * 3, Kr=list(COLOURS[k]) if which == "kr" else [1.0] * 3))
        elif which == "kt":
            prod.append(dict(base, Kr=GREY, kt_tex=TEX))
            orc.append(dict(base, Kr=GREY, Kt=list(COLOURS[k])))
        else:
            prod.append(dict(base, kr_tex=TEX, kt_tex=TEX_ROT))
            orc.append(dict(base, Kr=list(COLOURS[k]), Kt=list(COLOURS[(k + 1) % 4])))
    return prod, orc


def _pair(mpss, pbrtscene, which, spp=4, back_light=False, seed=3):
    """The product's context of a case, preprocessed, and the oracle's scene over the same points and irradiance
    (Kr and Kt reach neither)."""
    prod, orc = _case(which)
    sc = _quad_scene(pbrtscene, prod, spp, back_light)
    ctx = pbrtscene.build_context(sc)
    ctx.preprocess(seed=seed)
    o = orr.OracleScene(_quad_scene(pbrtscene, orc, spp, back_light), orr.tables_from_ctx(ctx, 4), ctx.cfg, mpss)
    o.set_octree(ctx.surface_points(), ctx.irradiance())
    return sc, ctx, o


def _quad_pixels(k):
    """A 7 x 7 pixel window well inside quad k's image (the quad spans about 16 pixels)."""
    sx, sy = [(-1, -1), (1, -1), (-1, 1), (1, 1)][k]
    r = OFF / Z / np.tan(np.radians(30.0)) * (W / 2)
    x, y = int(W / 2 + sx * r), int(H / 2 - sy * r)  # (raster y runs down)
    return slice(y - 3, y + 4), slice(x - 3, x + 4)


def test_block_lookups_are_the_block_colours(mpss):
    """The precondition of the parity tests: over each quad's uv range, with differentials of twice the quad's
    uv extent per pixel, every lookup is the block's colour within 4 ulp per channel (black: exactly)."""
    for tex, cols in ((TEX, COLOURS), (TEX_ROT, COLOURS[1:] + COLOURS[:1])):
        for k in range(4):
            u0, u1, v0, v1 = _uv_rect(k)
            u, v = np.meshgrid(np.linspace(u0, u1, 33), np.linspace(v0, v1, 33))
            uvd = np.zeros((u.size, 6), np.float32)
            uvd[:, 0], uvd[:, 1] = u.ravel(), v.ravel()
            npix = 2 * HALF / Z / np.tan(np.radians(30.0)) * (W / 2)  # the quad's width in pixels
            uvd[:, 2], uvd[:, 5] = 2 * (u1 - u0) / npix, 2 * (v1 - v0) / npix
            for d in (uvd, uvd * np.array([1, 1, 0, 0, 0, 0], np.float32), uvd[:, [0, 1, 4, 5, 2, 3]]):
                got = mpss.host_imagemap_lookup(tex, d)
                want = np.asarray(cols[k], np.float32)
                assert np.all(np.abs(got - want) <= 4 * np.spacing(want)), (k, np.abs(got - want).max())
                if not want.any():
                    assert not got.any()


@pytest.mark.parametrize("which,back", [("kr", False), ("kt", False), ("both", False), ("kt", True)],
                         ids=["kr", "kt", "both", "kt-backlit"])
def test_block_constant_texture_vs_oracle(mpss, oracle, which, back):
    import torch
    from mpss import pbrtscene
    sc, ctx, o = _pair(mpss, pbrtscene, which, back_light=back)
    got = _render_gpu(torch, ctx, sc, 0, W, 0, H, 23)
    ref = o.render_tile(sc.spp, 23, 0, W, 0, H)
    o.close()
    for k in range(4):
        # every quad is in view and lit, by Mo() if by nothing else; from behind, where the points face away from
        # the light, by the transmission lobe alone, which the black block's quad does not have
        assert (ref[_quad_pixels(k)][..., 1] > 0).all() != (back and k == 2)
    _check(got, ref)
    if which == "kr":
        # the texture is really applied: each quad (none is white) differs from its all-white-Kr render
        white = pbrtscene.build_context(_quad_scene(pbrtscene, _case("white")[0]))
        white.preprocess(seed=3)
        img = _render_gpu(torch, white, sc, 0, W, 0, H, 23)
        white.close()
        peak = np.abs(img[..., :3]).max()
        for k in range(4):
            d = np.abs(img[_quad_pixels(k)][..., :3] - got[_quad_pixels(k)][..., :3]).max()
            print("quad %d: max |white - textured| = %.3g of the peak" % (k, d / peak))
            assert d > 1e-3 * peak
    ctx.close()


def test_halo_path_vs_oracle_samples(mpss, oracle):
    """filter_pass.hip's copy of the lookups: gaussian film at spp 1 = the restated AddSample over the oracle's
    per-sample XYZ (test_pixel_filter_gpu.py test 2, its bounds)."""
    import torch
    from mpss import pbrtscene
    SEED, PARITY = 21, 1e-4
    sc, ctx, o = _pair(mpss, pbrtscene, "both", spp=1)
    o1 = o.render_tile(1, SEED, 0, W, 0, H)
    o.close()
    f = fr.describe("gaussian")
    R = fr.halo(f[1])
    bad = o1[..., 3] != 1  # an edge-rounded sample: the pixel's XYZ is not one sample's
    assert bad.mean() <= 0.01
    ctx.set_pixel_filter("gaussian")
    got = _render_gpu(torch, ctx, sc, 0, W, 0, H, SEED).astype(np.float64)
    ctx.close()
    px, py, X, Y = fr.image_positions(f, W, H, 1, SEED)
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    r = fr.add_samples(f, W, H, X[inside], Y[inside], o1[py[inside], px[inside], :3])
    keep = np.zeros((H, W), bool)
    keep[R:H - R, R:W - R] = True
    for y, x in zip(*np.nonzero(bad)):
        keep[max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1] = False
    assert keep.sum() >= 0.5 * W * H
    assert np.all(np.abs(got[..., 3] - r["film"][..., 3])[keep] <= (r["n"] * EPS * r["absw"])[keep])
    err = np.abs(got[..., :3] - r["film"][..., :3])
    tol = r["n"][..., None] * EPS * r["absx"] + PARITY * r["absx"]
    print("gaussian: worst err / tol %.3g on %d pixels" % ((err[keep] / np.maximum(tol[keep], 1e-300)).max(), keep.sum()))
    assert np.all(err[keep] <= tol[keep])
    assert (r["film"][keep][:, 1] > 0).mean() > 0.3


def _head(pbrtscene):
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "skin.pbrt"), xres=W, yres=H, spp=4)
    sc.integrator["minsampledistance"] = 0.008
    for m in sc.materials:
        m.update(desired_length=128, albedo_tex=ALBEDO, bump_tex=BUMP)
    return sc


def _close(a, b, name):
    """Test 3's bound: weights equal, |a - b| <= 1e-5 max(|b|, 1e-6 peak) on every XYZ value."""
    assert np.array_equal(a[..., 3], b[..., 3])
    peak = np.abs(b[..., :3]).max()
    assert peak > 0
    q = np.abs(a[..., :3].astype(np.float64) - b[..., :3]) / np.maximum(np.abs(b[..., :3]), 1e-6 * peak)
    print("%s: worst relative difference %.3g (bound 1e-5)" % (name, q.max()))
    assert q.max() <= 1e-5


@pytest.mark.parametrize("c", [(0.5, 0.25, 1.0), (0.0, 0.0, 0.0)], ids=["colour", "black"])
def test_constant_texture_is_the_constant_colour(mpss, c):
    import torch
    from mpss import pbrtscene
    imgs = []
    for textured in (False, True):
        sc = _head(pbrtscene)
        for m in sc.materials:
            m.pop("Kr", None)
            m.update(dict(kr_tex=dict(texels=np.full((4, 4, 3), c, np.float32))) if textured else dict(Kr=list(c)))
        ctx = pbrtscene.build_context(sc)
        ctx.preprocess(seed=3)
        imgs.append(_render_gpu(torch, ctx, sc, 0, W, 0, H, 23))
        ctx.close()
    const, tex = imgs
    assert (const[..., 1] > 0).mean() > 0.05
    if any(c):
        _close(tex, const, "Kr texture of equal texels vs color Kr")
    else:
        assert tex.tobytes() == const.tobytes()


def test_abi_entry_point_and_refusals(mpss):
    lib = mpss.lib()
    assert hasattr(lib, "mpss_set_material_spec_textures") and lib.mpss_abi_version() == 13
    ctx = mpss.Context()
    skin = ctx.add_layeredskin(mpss.default_skin(desired_length=64))
    colour = ctx.add_imagemap(**TEX)
    flt = ctx.add_imagemap(texels=TEX["texels"], is_float=True)
    dip = ctx.add_dipole_material(np.full(30, 0.1, np.float32), np.full(30, 1.0, np.float32), 1.3)
    for args in ((skin, flt, -1), (skin, -1, flt), (skin, 99, -1), (skin, -1, 99), (99, colour, -1),
                 (dip, colour, -1), (dip, -1, -1)):
        assert lib.mpss_set_material_spec_textures(ctx.h, *args) == -1, args  # MPSS_ERR_INVALID
        assert lib.mpss_last_error().decode().startswith("set_material_spec_textures: ")
    assert lib.mpss_set_material_spec_textures(ctx.h, skin, colour, colour) == 0
    assert lib.mpss_set_material_spec_textures(ctx.h, skin, -1, -1) == 0
    assert lib.mpss_set_material_spec_textures(None, skin, -1, -1) == -1
    ctx.close()


def test_bindings_survive_updates_and_count_in_n_tex(mpss):
    import torch
    from mpss import pbrtscene
    prod = _case("kr")[0]
    sc = _quad_scene(pbrtscene, prod)
    ctx = pbrtscene.build_context(sc)
    ctx.set_instrumentation(kernel_timing=True)
    ctx.preprocess(seed=3)
    ctx.reset_render_stats()
    first = _render_gpu(torch, ctx, sc, 0, W, 0, H, 23)
    n_tex = ctx.render_stats()["n_tex"]
    # mpss_set_material_textures leaves the Kr binding alone (the scene goes dirty: Preprocess again)
    ctx.set_material_textures(0, -1, -1)
    ctx.preprocess(seed=3)
    assert _render_gpu(torch, ctx, sc, 0, W, 0, H, 23).tobytes() == first.tobytes()
    # new pigments under the same ids: the texture still drives Kr
    new = [dict(m, f_mel=0.2, f_blood=0.8) for m in prod]
    for mid, m in enumerate(new):
        ctx.update_layeredskin(mid, pbrtscene.skin_struct(m))
    ctx.preprocess(seed=3)
    updated = _render_gpu(torch, ctx, sc, 0, W, 0, H, 23)
    ctx.close()
    fresh = pbrtscene.build_context(_quad_scene(pbrtscene, new))
    fresh.preprocess(seed=3)
    want = _render_gpu(torch, fresh, sc, 0, W, 0, H, 23)
    fresh.close()
    _close(updated, want, "update_layeredskin vs a fresh context")
    assert np.abs(updated[..., :3] - first[..., :3]).max() > 1e-3 * np.abs(first[..., :3]).max()  # (new pigments)
    # the same scene without the Kr texture launches no texture kernel at all
    plain = pbrtscene.build_context(_quad_scene(pbrtscene, _case("white")[0]))
    plain.set_instrumentation(kernel_timing=True)
    plain.preprocess(seed=3)
    plain.reset_render_stats()
    _render_gpu(torch, plain, sc, 0, W, 0, H, 23)
    n_plain = plain.render_stats()["n_tex"]
    plain.close()
    assert n_plain == 0 and n_tex > n_plain
