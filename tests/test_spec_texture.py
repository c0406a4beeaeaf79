"""LayeredSkin "texture Kr" / "texture Kt" without a GPU: the scene loader keeps a colour or spectrum
imagemap bound to Kr or Kt as kr_tex / kt_tex (the texture's mpss.imagemap keywords) beside albedo_tex,
still refuses a float texture, scenes/skin_spec.pbrt loads with its texels (its map is the tracked
tests/golden/skin_spec.tga), and
tools/make_textures.py's generators give the tracked TGAs byte for byte, the two older ones unchanged."""
import importlib.util
import os

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_KT = '"color Kr" [1 1 1] "color Kt" [0 0 0]'


def _scene_text(tmp_path, textures, bindings):
    """scenes/skin.pbrt with Texture lines before its Material and `bindings` in place of its constant Kr / Kt;
    tmp_path gets spec.tga (6 x 4)."""
    img = (synth.texture_texels(6, 4, seed=5) * 255).astype(np.uint8)
    hdr = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 0, 4, 0, 24, 0x20])  # top-left origin
    (tmp_path / "spec.tga").write_bytes(hdr + img[:, :, ::-1].tobytes())
    txt = open(os.path.join(ROOT, "scenes", "skin.pbrt")).read()
    assert KR_KT in txt
    txt = txt.replace('Material "layeredskin"', textures + '\n    Material "layeredskin"').replace(KR_KT, bindings)
    txt = txt.replace('"string npzfile" "head_mesh.npz"', '"string npzfile" "%s"' % os.path.join(
        ROOT, "scenes", "head_mesh.npz"))
    (tmp_path / "t.pbrt").write_text(txt)
    return str(tmp_path / "t.pbrt"), img


SPEC = ('Texture "spec" "%s" "imagemap" "string filename" "spec.tga" "string wrap" "clamp" "float gamma" 2.2 '
        '"float scale" 2')


@pytest.mark.parametrize("typ", ["color", "spectrum"])
def test_loader_keeps_kr_imagemap(mpss, tmp_path, typ):
    from mpss import pbrtscene
    path, img = _scene_text(tmp_path, SPEC % typ, '"texture Kr" "spec" "color Kt" [0 0 0]')
    m = pbrtscene.load(path).materials[0]
    t = m["kr_tex"]
    assert (t["wrap"], t["gamma"], t["scale"], t["shift"], t["is_float"]) == ("clamp", 2.2, 2.0, 0.0, False)
    assert (t["trilinear"], t["maxanisotropy"], t["uscale"], t["vdelta"]) == (False, 8.0, 1.0, 0.0)
    np.testing.assert_allclose(t["texels"], img[::-1] / 255.0, atol=1e-6)  # (ReadImageTGA: bottom row first)
    assert "Kr" not in m and "kt_tex" not in m and m["Kt"] == [0.0, 0.0, 0.0]
    # the texture bindings are no fields of mpss_layeredskin: the struct builds without them
    assert set(pbrtscene.TEXTURE_KEYS) == {"albedo_tex", "bump_tex", "kr_tex", "kt_tex"}
    skin = pbrtscene.skin_struct(m)
    assert list(skin.Kt) == [0.0] * 30


def test_loader_keeps_kt_imagemap_and_both(mpss, tmp_path):
    from mpss import pbrtscene
    two = SPEC % "color" + '\n    Texture "thru" "color" "imagemap" "string filename" "spec.tga" "float scale" 0.25'
    path, _ = _scene_text(tmp_path, two, '"color Kr" [0.5 0.5 0.5] "texture Kt" "thru"')
    m = pbrtscene.load(path).materials[0]
    assert m["kt_tex"]["scale"] == 0.25 and m["kt_tex"]["wrap"] == "repeat" and m["kt_tex"]["texels"].shape == (4, 6, 3)
    assert "kr_tex" not in m and m["Kr"] == [0.5, 0.5, 0.5]
    path, _ = _scene_text(tmp_path, two, '"texture Kr" "spec" "texture Kt" "thru"')
    m = pbrtscene.load(path).materials[0]
    assert m["kr_tex"]["gamma"] == 2.2 and m["kt_tex"]["scale"] == 0.25
    pbrtscene.skin_struct(m)


@pytest.mark.parametrize("key", ["Kr", "Kt"])
def test_loader_refuses_float_texture(mpss, tmp_path, key):
    from mpss import pbrtscene
    path, _ = _scene_text(tmp_path, SPEC % "float", '"texture %s" "spec"' % key)
    with pytest.raises(ValueError, match="%s needs a spectrum texture, 'spec' is a float texture" % key):
        pbrtscene.load(path)


def _make_textures():
    spec = importlib.util.spec_from_file_location("make_textures", os.path.join(ROOT, "tools", "make_textures.py"))
    mt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mt)
    return mt


def test_skin_spec_scene_loads(mpss):
    from mpss import pbrtscene
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "skin_spec.pbrt"))
    ref = pbrtscene.load(os.path.join(ROOT, "scenes", "skin_textured.pbrt"))
    m = sc.materials[0]
    t = m["kr_tex"]
    assert (t["wrap"], t["gamma"], t["scale"]) == ("clamp", 2.2, 2.0)  # as the fork's GT007 "spec" texture
    assert t["texels"].shape == (256, 256, 3)
    black = (t["texels"] == 0).all(axis=2)
    assert 0.2 < black.mean() < 0.3 and t["texels"][~black].min() > 0.4  # exact zeros, nothing merely dark
    assert m["Kt"] == [0.0, 0.0, 0.0] and "Kr" not in m
    # everything else is skin_textured.pbrt
    assert (sc.xres, sc.yres, sc.spp, sc.integrator) == (ref.xres, ref.yres, ref.spp, ref.integrator)
    r = ref.materials[0]
    assert np.array_equal(m["albedo_tex"]["texels"], r["albedo_tex"]["texels"])
    assert np.array_equal(m["bump_tex"]["texels"], r["bump_tex"]["texels"])
    assert {k: v for k, v in m.items() if not k.endswith("_tex")} == {
        k: v for k, v in r.items() if not k.endswith("_tex") and k != "Kr"}


def test_make_textures_keeps_the_old_files(tmp_path):
    """The tracked TGAs are the generators' bytes: the two older files (which this change does not touch) and
    the spec map, tests/golden/skin_spec.tga, that scenes/skin_spec.pbrt names; the tool writes exactly those."""
    mt = _make_textures()
    alb, bump = mt.albedo_and_bump()
    tex = os.path.join(ROOT, "scenes", "textures")
    old = {n: open(os.path.join(tex, n), "rb").read() for n in ("skin_albedo.tga", "skin_bump.tga")}
    assert mt.tga_bytes(alb) == old["skin_albedo.tga"]
    assert mt.tga_bytes(bump) == old["skin_bump.tga"]
    spec = open(os.path.join(ROOT, "tests", "golden", "skin_spec.tga"), "rb").read()
    assert mt.tga_bytes(mt.spec()) == spec and len(spec) == 18 + 256 * 256 * 3
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    mt.main(str(tmp_path / "a"), str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(old) and os.listdir(tmp_path / "b") == ["skin_spec.tga"]
    assert all((tmp_path / "a" / n).read_bytes() == old[n] for n in old)
    assert (tmp_path / "b" / "skin_spec.tga").read_bytes() == spec
