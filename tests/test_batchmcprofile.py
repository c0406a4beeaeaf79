"""The "batchmcprofile" renderer's host side (mpss/batchmcprofile.py, BatchMCProfileRenderer,
src/renderers/batchmcprofile.cpp:43-141): the thickness list, the parameter factory and its errors, the
loader, the table writer and reader, and the two batch entry points' argument checks. CPU-only."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "scenes", "batchmcprofile.pbrt")
LAYERS = [(723.6646118164062, 577.9549560546875, 1.399999976158142, 0.0024999999441206455),
          (9.664658546447754, 288.97747802734375, 1.399999976158142, 0.20000000298023224)]
HEADER = ("Thickness\tMonte-Carlo Reflectance\tMultipole Reflectance\tLerped Reflectance"
          "\tMonte-Carlo Transmittance\tMultipole Transmittance\tLerped Transmittance")


def _params(mpss, **kw):
    from mpss import pbrtscene
    ps = pbrtscene.ParamSet()
    for k, v in kw.items():
        ps[k] = ("x", list(v) if isinstance(v, (list, tuple)) else [v])
    return ps


@pytest.mark.parametrize("lo,hi,n", [(0.00001, 0.005, 256), (0.25, 0.25, 4), (1, 2, 1)])
def test_thicknesses_in_float32(mpss, lo, hi, n):
    from mpss import batchmcprofile
    r = batchmcprofile.BatchMCProfileRenderer(LAYERS, thickness_min=lo, thickness_max=hi, thickness_segments=n)
    got = r.thicknesses()
    f = np.float32
    want = [f(lo) + f(f(ii) * f(f(hi) - f(lo))) / f(n) for ii in range(n + 1)]  # batchmcprofile.cpp:54
    assert got.dtype == np.float32 and len(got) == n + 1
    assert all(type(w) is np.float32 for w in want)
    assert np.array_equal(got, np.array(want, np.float32))
    assert np.all(np.diff(got) >= 0) and got[0] == f(lo)
    s = r.slabs()
    assert s.shape == (n + 1, 2, 4) and np.array_equal(s[:, 0, 3], got)
    assert np.array_equal(s[:, 1], np.repeat(np.asarray(LAYERS, np.float32)[None, 1], n + 1, axis=0))


def test_create_from_params_defaults(mpss):
    from mpss import batchmcprofile
    flat = [x for l in LAYERS for x in l]
    r = batchmcprofile.create_from_params(_params(mpss, layers=flat, thicknessrange=[0.001, 0.002]))
    assert (r.mfp_range, r.segments, r.thickness_segments, r.photons, r.filename) == (16.0, 1024, 256, 100, "")
    assert r.thickness_min == float(np.float32(0.001)) and r.thickness_max == float(np.float32(0.002))
    assert r.layers.shape == (2, 4)
    r = batchmcprofile.create_from_params(_params(mpss, layers=flat, thicknessrange=[0.0, 0.0], mfprange=12.0,
                                                  segments=64, thicknesssegments=4, photons="5000",
                                                  filename="t.txt"))
    assert (r.mfp_range, r.segments, r.thickness_segments, r.photons, r.filename) == (12.0, 64, 4, 5000, "t.txt")


@pytest.mark.parametrize("tr", [None, [0.001], [0.002, 0.001], [-0.001, 0.001], [0.001, 0.002, 0.003]])
def test_create_from_params_bad_thickness_range(mpss, tr):
    from mpss import batchmcprofile
    kw = dict(layers=[x for l in LAYERS for x in l])
    if tr is not None:
        kw["thicknessrange"] = tr
    with pytest.raises(ValueError, match="Thickness range incorrectly set for BatchMCProfileRenderer."):
        batchmcprofile.create_from_params(_params(mpss, **kw))


def test_create_from_params_needs_layers(mpss):
    from mpss import batchmcprofile
    with pytest.raises(ValueError, match="No layers param set for BatchMCProfileRenderer."):
        batchmcprofile.create_from_params(_params(mpss, thicknessrange=[0.001, 0.002]))


def test_loader_accepts_the_scene(mpss, tmp_path):
    from mpss import batchmcprofile, pbrtscene
    assert "reconstruction" in open(SCENE).read().split("Renderer")[0]
    sc = pbrtscene.load(SCENE)
    assert sc.renderer[0] == "batchmcprofile"
    r = batchmcprofile.create_from_params(sc.renderer[1])
    assert np.array_equal(r.layers, np.asarray(LAYERS, np.float32))
    assert (r.segments, r.thickness_segments, r.photons, r.filename) == (256, 256, 1000000, "batchmcprofile.txt")
    th = r.thicknesses()
    assert len(th) == 257 and th[0] == np.float32(0.00001) and abs(float(th[-1]) - 0.005) < 1e-9
    bad = tmp_path / "bad.pbrt"
    bad.write_text('Renderer "metropolis"\nWorldBegin\nWorldEnd\n')
    with pytest.raises(ValueError, match="outside this path"):
        pbrtscene.load(str(bad))


def test_tsv_round_trip(mpss, tmp_path):
    from mpss import batchmcprofile
    res = [dict(thickness=1e-05, totalMCReflectance=0.123456789, totalNoLerpReflectance=0.5,
                totalLerpReflectance=1.0 / 3.0, totalMCTransmittance=2.5e-07, totalNoLerpTransmittance=0.0,
                totalLerpTransmittance=1234567.0),
           dict(thickness=0.0025, totalMCReflectance=0.25, totalNoLerpReflectance=0.26,
                totalLerpReflectance=0.27, totalMCTransmittance=0.011, totalNoLerpTransmittance=0.012,
                totalLerpTransmittance=0.013)]
    txt = batchmcprofile.tsv(res)
    lines = txt.split("\n")
    assert txt.endswith("\n") and lines[0] == HEADER and len(lines) == 4 and lines[3] == ""
    assert lines[1] == "1e-05\t0.123457\t0.5\t0.333333\t2.5e-07\t0\t1.23457e+06"
    assert lines[2] == "0.0025\t0.25\t0.26\t0.27\t0.011\t0.012\t0.013"
    p = tmp_path / "t.txt"
    p.write_bytes(txt.encode())
    back = batchmcprofile.read_tsv(str(p))
    assert len(back) == 2 and list(back[0]) == list(res[0])
    for a, b in zip(back, res):
        for k in b:
            assert a[k] == float("%g" % b[k])  # exact at the six digits written
    assert batchmcprofile.tsv(back) == txt


def test_batch_entry_points_check_arguments_without_a_device(mpss):
    L = mpss.lib()
    lay = np.asarray([LAYERS, LAYERS], np.float32)
    tr, tt = np.zeros(2), np.zeros(2)
    fake = C.create_string_buffer(64)  # never dereferenced: the argument checks come first
    ctx = C.addressof(fake)
    walk = lambda c, l, s, r, t: L.mpss_mc_profile_batch(c, l, s, 2, 16.0, 8, 10, 89, None, None, r, t, None, None)
    ref = lambda c, l, s, r, t: L.mpss_mc_reference_batch(c, l, s, 2, 16.0, 8, 64, 1, 0, None, None, r, t, None)
    for f, name in ((walk, b"mpss_mc_profile_batch"), (ref, b"mpss_mc_reference_batch")):
        for args in ((None, lay.ctypes.data, 2, tr.ctypes.data, tt.ctypes.data),
                     (ctx, None, 2, tr.ctypes.data, tt.ctypes.data),
                     (ctx, lay.ctypes.data, 2, None, tt.ctypes.data),
                     (ctx, lay.ctypes.data, 2, tr.ctypes.data, None)):
            assert f(*args) != 0
            assert name in L.mpss_last_error() and b"null" in L.mpss_last_error()
        assert f(ctx, lay.ctypes.data, 0, tr.ctypes.data, tt.ctypes.data) != 0
        assert name in L.mpss_last_error() and b"slabs" in L.mpss_last_error()
