"""The GPU common-grid builder (mpss_set_grid_builder(ctx, 0): csrc/common_grid_gpu.hip scans every band
knot on the device) must build the host builder's grid bit for bit: Context.common_grid(mid, nf), the grid
the context built, against mpss.host_common_grid of the same table, field for field and with the rows as
uint32 bit patterns (the NaN flag's pattern included), for both LDS layouts.

Cases: the smallest tables that reach each branch of build_common_grid (csrc/common_grid.cpp; both
builders compute through csrc/common_grid_math.h), installed with
set_material_tables, and LayeredSkin materials built by add_layeredskin. One more case renders a tissue
window with the GPU-built and with the host-built grid: the same film bytes.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("rows", "bands", "rg", "u0lim", "u1lim", "u1start", "row0", "ubase", "rel_err", "l1_err", "ua", "hinv")


def _same_grid(got, want, what):
    assert got["ok"] == want["ok"], what
    for k in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, k)


def _gpu_ctx(mpss, **cfg):
    ctx = mpss.Context(**cfg)
    ctx.set_grid_builder(on_host=False)
    return ctx


def _tables():
    rng = np.random.default_rng(5)
    out = {}
    out["L3"] = (np.ones((30, 3), np.float32), np.full(30, 100.0, np.float32), False)
    rcp0 = np.full(30, 99.0 / 0.004, np.float32)
    rcp0[7] = 0.0
    x = np.linspace(0, 1, 100, dtype=np.float32)
    out["zero_rcp"] = (np.stack([np.exp(-x * (4 + 0.2 * c)) for c in range(30)]).astype(np.float32), rcp0, False)
    x = np.linspace(0, 1, 4, dtype=np.float32)
    out["L4"] = (np.stack([np.exp(-x * (4 + 0.2 * c)) for c in range(30)]).astype(np.float32),
                 np.full(30, 3.0 / 0.004, np.float32), None)
    L = 4096  # test_common_grid_of_a_rough_table (tests/test_common_grid.py)
    x = np.arange(L) / L
    out["rough"] = (np.stack([np.exp(-x * (3 + c)) * (1 + 0.3 * rng.random(L)) for c in range(30)]).astype(np.float32),
                    ((L - 1) / np.linspace(0.01, 0.05, 30)).astype(np.float32), True)
    L = 30000
    x = np.linspace(0, 1, L, dtype=np.float32)
    out["equal"] = (np.stack([np.exp(-x * (4 + 0.2 * c)) for c in range(30)]).astype(np.float32),
                    np.full(30, (L - 1) / 0.004, np.float32), True)
    L = 6000
    x = np.linspace(0, 1, L)
    out["smooth"] = (np.stack([np.exp(-x * (5 + 0.3 * c)) for c in range(30)]).astype(np.float32),
                     ((L - 1) / np.linspace(0.002, 0.006, 30)).astype(np.float32), True)
    return out


@pytest.mark.parametrize("name", ["L3", "zero_rcp", "L4", "rough", "equal", "smooth"])
def test_installed_tables(mpss, name):
    tab, rcp, ok = _tables()[name]
    ctx = _gpu_ctx(mpss)
    mid = ctx.set_material_tables(tab, rcp, np.zeros(1025, np.float32))
    for nf in (5088, 10236):
        got = ctx.common_grid(mid, nf)
        want = mpss.host_common_grid(tab, rcp, near_field=nf)
        if ok is not None:
            assert want["ok"] == ok, "the case no longer reaches its branch"
        if ok is False:  # both builders decline: no rows, the per-band tables are used
            assert not got["ok"] and len(got["rows"]) == 0 and not ctx.gather_info(mid)["common_grid"]
            continue
        _same_grid(got, want, (name, nf))
        if name == "equal":  # every band on the group grid: the rows are the tables
            assert want["ok"] and float(want["rel_err"].max()) == 0.0
        if name == "rough":
            assert np.isnan(want["rows"][:, 0]).any()  # flagged cells
    ctx.close()


SKINS = {
    "golden64": (dict(desired_length=64), {}),
    "default512": (dict(desired_length=512), {}),
    "low_absorption": (dict(f_blood=0.0, f_mel=0.0, f_eu=0.0, layer_thickness_nm=[0.03e6, 20e6], roughness=0.35,
                            nmperunit=40e6, f_ohg=0.75), {}),
    "low_absorption_rgb": (dict(f_blood=0.0, f_mel=0.0, f_eu=0.0, layer_thickness_nm=[0.03e6, 20e6], roughness=0.35,
                                nmperunit=40e6, f_ohg=0.75, rgb_profile=1), {}),
    "snake": (dict(desired_length=512), dict(mo_band_dealing=1)),
}


@pytest.mark.parametrize("name", sorted(SKINS))
def test_layeredskin_materials(mpss, name):
    skin, cfg = SKINS[name]
    ctx = _gpu_ctx(mpss, **cfg)
    mid = ctx.add_layeredskin(mpss.default_skin(**skin))
    tab, rcp, _, _ = ctx.material_tables(mid)
    rgb = bool(skin.get("rgb_profile"))
    for nf in (5088, 10236):
        got = ctx.common_grid(mid, nf)
        want = mpss.host_common_grid(tab, rcp, snake=bool(cfg.get("mo_band_dealing")), rgb=rgb, near_field=nf)
        assert want["ok"]
        _same_grid(got, want, (name, nf))
        if name == "default512":  # L ~ 120 k: the row cap is reached with rows H = 2 or 4 apart
            assert tab.shape[1] > 100_000 and float(want["hinv"].min()) < 1.0
    ctx.close()


def test_tissue_window_with_either_builder(mpss):
    import torch
    from mpss import pbrtscene
    from test_configs_gpu import _windows
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "tissue.pbrt"))
    films = []
    win = None
    for on_host in (True, False):
        ctx = _build_with_builder(mpss, sc, on_host)
        ctx.preprocess(seed=1)
        assert ctx.gather_info(0)["common_grid"]
        if win is None:
            win = _windows(ctx, sc.xres, sc.yres, 32, 32, lambda f: f == 1.0)
        x0, x1, y0, y1 = win
        out = torch.zeros((32 * 32 * 4,), dtype=torch.float32, device="cuda")
        ctx.render_tile(sc.spp, 9, x0, x1, y0, y1, out.data_ptr())
        torch.cuda.synchronize()
        films.append(out.cpu().numpy().tobytes())
        ctx.close()
    assert films[0] == films[1]


def _build_with_builder(mpss, sc, on_host):
    """pbrtscene.build_context with the grid builder chosen first: the scene's context, then its material
    rebuilt in place under the chosen builder (update_layeredskin builds what add_layeredskin does)."""
    from mpss import pbrtscene
    ctx = pbrtscene.build_context(sc)
    ctx.set_grid_builder(on_host)
    ctx.update_layeredskin(0, pbrtscene.skin_struct(sc.materials[0]))
    return ctx
