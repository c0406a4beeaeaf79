"""mpss_update_layeredskin: a material rebuilt in place must leave the context exactly where a fresh
context with that material stands -- film, tables, irradiance, surface points, gather info and common
grids byte for byte -- while the scene upload and the surface point set are reused (mpss_build_counts),
renders between the update and the next Preprocess are refused, and in-flight renders finish on the
old material.

Scene: scenes/tissue.pbrt (C1: 256 x 256, 8 spp), one 32 x 32 all-skin window. P0 is the scene's own
material; P1, P2 are rows of tests/golden/perms_first16.csv (the first rows of the fork's
utilities/csv/perms.csv) through mpss.sweep.pigment_skin. Fresh contexts are built once per
(material, sampler) and shared.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(ROOT, "tests", "golden", "perms_first16.csv")
SEED, RSEED = 1, 9
_cache = {}


def _scene():
    from mpss import pbrtscene
    if "scene" not in _cache:
        _cache["scene"] = pbrtscene.load(os.path.join(ROOT, "scenes", "tissue.pbrt"))
    return _cache["scene"]


def _mat(which, **over):
    from mpss import sweep
    base = _scene().materials[0]
    rows = sweep.read_rows(CSV)
    m = dict(base) if which == 0 else sweep.pigment_skin(base, *rows[{1: 3, 2: 13}[which]])
    m.update(over)
    return m


def _build(mat, **cfg):
    from mpss import pbrtscene
    sc = _scene()
    mats = sc.materials
    sc.materials = [mat]
    try:
        return pbrtscene.build_context(sc, **cfg)
    finally:
        sc.materials = mats


def _window(ctx):
    if "win" not in _cache:
        from test_configs_gpu import _windows
        sc = _scene()
        _cache["win"] = _windows(ctx, sc.xres, sc.yres, 32, 32, lambda f: f == 1.0)
    return _cache["win"]


def _render(ctx, stream=None, sync=True):
    import torch
    x0, x1, y0, y1 = _window(ctx)
    out = torch.zeros(((y1 - y0) * (x1 - x0) * 4,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.render_tile(_scene().spp, RSEED, x0, x1, y0, y1, out.data_ptr(), stream)
    if not sync:
        return out
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _state(ctx):
    """Everything the issue lists, as bytes (preprocessed context)."""
    st = dict(film=_render(ctx).tobytes())
    for k, v in zip(("table", "rcp", "rho", "total"), ctx.material_tables(0)):
        st[k] = v.tobytes()
    st["irradiance"] = ctx.irradiance().tobytes()
    st["points"] = ctx.surface_points().tobytes()
    gi = ctx.gather_info(0)
    st["gather"] = (gi["common_grid"], gi["rel_err"].tobytes(), gi["l1_err"].tobytes())
    for nf in (5088, 10236):
        cg = ctx.common_grid(0, nf)
        st["grid%d" % nf] = tuple((k, np.asarray(cg[k]).tobytes()) for k in sorted(cg))
    return st


def _fresh_state(key, mat, **cfg):
    """The state of a fresh context with `mat` (built once per key)."""
    k = ("fresh", key, tuple(sorted(cfg.items())))
    if k not in _cache:
        ctx = _build(mat, **cfg)
        ctx.preprocess(seed=SEED)
        _cache[k] = _state(ctx)
        ctx.close()
    return _cache[k]


def _assert_same(got, want, what):
    for k in want:
        assert got[k] == want[k], "%s: %s differs from a fresh context's" % (what, k)


def _skin(mat):
    from mpss import pbrtscene
    return pbrtscene.skin_struct(mat)


@pytest.mark.parametrize("sampler", ["hash", "reference"])
def test_update_equals_fresh(mpss, sampler):
    cfg = dict(sampler=mpss.SAMPLER_REFERENCE if sampler == "reference" else mpss.SAMPLER_HASH)
    a = _build(_mat(0), **cfg)
    a.preprocess(seed=SEED)
    _assert_same(_state(a), _fresh_state("P0", _mat(0), **cfg), "P0")
    for which in (1, 2):  # (the second update: from an updated state)
        a.update_layeredskin(0, _skin(_mat(which)))
        a.preprocess(seed=SEED)
        got = _state(a)
        want = _fresh_state("P%d" % which, _mat(which), **cfg)
        _assert_same(got, want, "update to P%d" % which)
        assert got["film"] != _fresh_state("P0", _mat(0), **cfg)["film"]  # (the pigments do change the frame)
    a.close()


def test_reuse_is_real(mpss):
    a = _build(_mat(0))
    a.preprocess(seed=SEED)
    _render(a)
    c0 = a.build_counts()
    assert c0 == dict(scene_uploads=1, point_builds=1, material_builds=1, octree_builds=1)
    a.update_layeredskin(0, _skin(_mat(1)))
    a.preprocess(seed=SEED)
    _render(a)
    c1 = a.build_counts()
    delta = {k: c1[k] - c0[k] for k in c0}
    assert delta == dict(scene_uploads=0, point_builds=0, material_builds=1, octree_builds=1)
    # a geometry change instead: the scene is uploaded and the points are found again
    me = _scene().meshes[0]
    a.add_mesh(me["P"] + np.float32([0, 0, 0.5]), me["indices"], me["o2w"], me["w2o"], 0, N=me["N"], S=me["S"],
               uv=me["uv"], reverse=me["reverse"])
    a.preprocess(seed=SEED)
    _render(a)
    c2 = a.build_counts()
    assert c2["scene_uploads"] == c1["scene_uploads"] + 1 and c2["point_builds"] == c1["point_builds"] + 1
    assert c2["material_builds"] == c1["material_builds"] and c2["octree_builds"] == c1["octree_builds"] + 1
    a.close()


def test_stale_state_is_an_error(mpss):
    import torch
    a = _build(_mat(0))
    a.preprocess(seed=SEED)
    x0, x1, y0, y1 = _window(a)
    a.update_layeredskin(0, _skin(_mat(1)))
    out = torch.zeros((32 * 32 * 4,), dtype=torch.float32, device="cuda")
    rc = mpss.lib().mpss_render_tile(a.h, _scene().spp, RSEED, x0, x1, y0, y1, out.data_ptr(), None)
    assert rc == -1  # MPSS_ERR_INVALID
    assert b"preprocess" in mpss.lib().mpss_last_error()
    with pytest.raises(mpss.MpssError, match="preprocess"):
        a.tile_costs([(x0, x1, y0, y1)])
    a.preprocess(seed=SEED)
    assert _render(a).tobytes() == _fresh_state("P1", _mat(1))["film"]
    a.close()


def test_switches(mpss):
    """rgbprofile, genprofile off and back, showirradiancepoints: each update equals a fresh context
    (a genprofile flip drops the cached point set; every one replaces the band layout)."""
    a = _build(_mat(0))
    a.preprocess(seed=SEED)
    steps = [("rgb", dict(rgb_profile=1)), ("nogen", dict(gen_profile=0)), ("P0", {}),
             ("showirr", dict(show_irradiance_points=1))]
    for key, over in steps:
        a.update_layeredskin(0, _skin(_mat(0, **over)))
        a.preprocess(seed=SEED)
        _assert_same(_state(a), _fresh_state(key, _mat(0, **over)), key)
    a.close()


def test_bad_targets(mpss):
    a = _build(_mat(0))
    dip = a.add_dipole_material(np.full(30, 0.01, np.float32), np.full(30, 1.0, np.float32), 1.3)
    a.preprocess(seed=SEED)
    want = _render(a).tobytes()
    skin = _skin(_mat(1))
    import ctypes as C
    for mid in (17, dip):
        rc = mpss.lib().mpss_update_layeredskin(a.h, mid, C.byref(skin))
        assert rc == -1 and mpss.lib().mpss_last_error()
    assert b"dipole" in mpss.lib().mpss_last_error()
    assert _render(a).tobytes() == want  # still renders, still P0
    a.close()


@pytest.mark.parametrize("exact", [0, 1])
def test_mo_batch_after_update(mpss, exact):
    import torch
    import synth
    radii = (0.05, 0.06, 0.07)
    cloud = synth.ellipsoid_cloud(2000, radii=radii, seed=3)
    q = torch.from_numpy(synth.surface_queries(256, radii=radii, seed=4)).cuda()
    p0 = mpss.default_skin(desired_length=64)
    p1 = _skin(dict(_mat(1), desired_length=64))

    def gather(ctx, mid):
        out = torch.zeros((256, 30), dtype=torch.float32, device="cuda")
        ctx.mo_batch(mid, 256, q.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    a = mpss.Context(max_error=0.1, exact_mo=exact)
    mid = a.add_layeredskin(p0)
    a.set_irradiance_points(*cloud)
    before = gather(a, mid)
    a.update_layeredskin(mid, p1)
    got = gather(a, mid)  # the caller's points: no Preprocess is involved
    b = mpss.Context(max_error=0.1, exact_mo=exact)
    mb = b.add_layeredskin(p1)
    b.set_irradiance_points(*cloud)
    want = gather(b, mb)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != before.tobytes() and np.abs(want).max() > 0
    a.close()
    b.close()


def test_update_waits_for_queued_render(mpss):
    """A render queued on a side stream still reads P0's tables; the update is ordered after it."""
    import torch
    a = _build(_mat(0))
    a.preprocess(seed=SEED)
    _window(a)
    s = torch.cuda.Stream()
    out = _render(a, stream=s.cuda_stream, sync=False)
    a.update_layeredskin(0, _skin(_mat(1)))  # (no synchronisation in between)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == _fresh_state("P0", _mat(0))["film"]
    a.preprocess(seed=SEED)
    assert _render(a).tobytes() == _fresh_state("P1", _mat(1))["film"]
    a.close()


def test_common_grid_export_is_the_host_grid(mpss):
    """mpss_get_common_grid hands out the grid the material build made: for both LDS layouts the host
    builder's grid of the same tables, field for field (rows as bit patterns)."""
    a = mpss.Context()
    mid = a.add_layeredskin(mpss.default_skin(desired_length=64))
    tab, rcp, _, _ = a.material_tables(mid)
    for nf in (5088, 10236):
        got = a.common_grid(mid, nf)
        want = mpss.host_common_grid(tab, rcp, near_field=nf)
        assert got["ok"] and sorted(got) == sorted(want)
        for k in want:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (nf, k)
    # a table too short for a grid: both decline
    L = 3
    t3 = np.ones((30, L), np.float32)
    m3 = a.set_material_tables(t3, np.full(30, 100.0, np.float32), np.zeros(1025, np.float32))
    got = a.common_grid(m3, 5088)
    assert not got["ok"] and len(got["rows"]) == 0
    assert not mpss.host_common_grid(t3, np.full(30, 100.0, np.float32))["ok"]
    a.close()
