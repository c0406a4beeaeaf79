"""Pigment sweeps: one scene rendered many times with different LayeredSkin pigments.

The fork templates a scene per row of a csv with columns H, M, E, B -- blood fraction, melanin
fraction, epidermis thickness (x 1e6 nm) and eumelanin fraction (utilities/python/SceneMaker.py:
6-62 over utilities/csv/perms.csv). Geometry, lights and camera are the same in every row, so a
context is built once and each row only rebuilds the material (Context.update_layeredskin), runs
Preprocess again (its surface points are reused; irradiance and octree are rebuilt) and renders.
"""
import csv
import time

import numpy as np

COLUMNS = ("H", "M", "E", "B")


def pigment_skin(base, H, M, E, B):
    """A material dict (as pbrtscene.Scene.materials holds them) with one csv row's pigments, the
    mapping of SceneMaker.py:40-51: "skinlayer layers" [E e6 1.4 20e6 1.4], f_mel = M, f_eu = B,
    f_blood = H. Everything else stays as in `base`."""
    m = dict(base)
    lay = list(base.get("layer_thickness_nm", [0.25e6, 20e6]))
    m.update(f_blood=float(H), f_mel=float(M), f_eu=float(B), layer_thickness_nm=[float(E) * 1e6, float(lay[1])])
    return m


def read_rows(path, limit=None):
    """The (H, M, E, B) rows of a pigment csv. Columns are found by the header's names (a byte-order
    mark is tolerated); a row with an empty cell in one of the four is skipped -- the fork's sampling
    tables pad their shorter columns with empty cells (PigmentSamplingValuesWThickness.csv), which
    SceneMaker.py drops as well."""
    rows = []
    with open(path, newline="", encoding="utf-8-sig") as f:
        rd = csv.reader(f)
        header = [h.strip() for h in next(rd)]
        idx = [header.index(c) for c in COLUMNS]
        for rec in rd:
            cells = [rec[i].strip() if i < len(rec) else "" for i in idx]
            if not all(cells):
                continue
            rows.append(tuple(float(c) for c in cells))
            if limit is not None and len(rows) >= limit:
                break
    return rows


def _sync():
    import torch
    torch.cuda.synchronize()


def render_frame(ctx, sc, seed=7, tile=256, out=None, spectral=False):
    """The whole frame in tile x tile rectangles (one mpss_render_tiles call) -> [H, W, 4] XYZW. spectral:
    one mpss_render_tiles_spectral call -> (XYZW, [H, W, 32] band sums, weight sum and 0 per pixel:
    film.finalize_spectral's input)."""
    import torch
    from mpss import tiles
    rects = tiles.tile_grid(sc.xres, sc.yres, tile)
    bufs = [torch.zeros(((r[3] - r[2]) * (r[1] - r[0]) * 4,), dtype=torch.float32, device="cuda") for r in rects]
    if spectral:
        sbufs = [torch.zeros(((r[3] - r[2]) * (r[1] - r[0]) * 32,), dtype=torch.float32, device="cuda") for r in rects]
        ctx.render_tiles_spectral(sc.spp, seed, rects, [b.data_ptr() for b in sbufs], [b.data_ptr() for b in bufs])
    else:
        ctx.render_tiles(sc.spp, seed, rects, [b.data_ptr() for b in bufs])
    torch.cuda.synchronize()
    film = np.zeros((sc.yres, sc.xres, 4), np.float32) if out is None else out
    for (x0, x1, y0, y1), b in zip(rects, bufs):
        film[y0:y1, x0:x1] = b.cpu().numpy().reshape(y1 - y0, x1 - x0, 4)
    if not spectral:
        return film
    spec = np.zeros((sc.yres, sc.xres, 32), np.float32)
    for (x0, x1, y0, y1), b in zip(rects, sbufs):
        spec[y0:y1, x0:x1] = b.cpu().numpy().reshape(y1 - y0, x1 - x0, 32)
    return film, spec


def sweep(sc, rows, mode="update", material=0, seed=1, render_seed=7, tile=256, grid_on_host=None, spectral=False,
          **cfg_kw):
    """Generator over rows of (H, M, E, B): yields (film [H, W, 4] XYZW, seconds, ctx) per row. seconds
    holds setup_s (building a context: scene, BVH upload aside, and its material; 0 for rows that
    build none), material_s (the material's table build), preprocess_s and render_s. mode "update":
    one context, built from the scene as it is, the material rebuilt in place for every row; "fresh":
    a new context per row with the row's material (all a library without mpss_update_layeredskin can
    do), material_s then being the part of setup_s spent in mpss_add_layeredskin. ctx is the context
    that rendered the row (valid until the generator is advanced). grid_on_host: the common-grid
    builder of the material builds (Context.set_grid_builder; None: the library's default). spectral: every
    row renders the band cube beside the film, and `film` is render_frame's pair (XYZW, [H, W, 32])."""
    from mpss import pbrtscene
    if mode not in ("update", "fresh"):
        raise ValueError("mode must be 'update' or 'fresh'")
    base = sc.materials[material]
    ctx = None
    try:
        for row in rows:
            secs = dict(setup_s=0.0)
            mat = pigment_skin(base, *row)
            if mode == "fresh":
                if ctx is not None:
                    ctx.close()
                    ctx = None
                mats = sc.materials
                sc.materials = mats[:material] + [mat] + mats[material + 1:]
                try:
                    timings = {}
                    t0 = time.perf_counter()
                    ctx = pbrtscene.build_context(sc, timings=timings, grid_on_host=grid_on_host, **cfg_kw)
                    secs["setup_s"] = time.perf_counter() - t0
                    secs["material_s"] = timings["material_s"]
                finally:
                    sc.materials = mats
            else:
                if ctx is None:
                    t0 = time.perf_counter()
                    ctx = pbrtscene.build_context(sc, grid_on_host=grid_on_host, **cfg_kw)
                    secs["setup_s"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                ctx.update_layeredskin(material, pbrtscene.skin_struct(mat))
                secs["material_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            ctx.preprocess(seed=seed)
            _sync()
            secs["preprocess_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            film = render_frame(ctx, sc, render_seed, tile, spectral=spectral)
            secs["render_s"] = time.perf_counter() - t0
            yield film, secs, ctx
    finally:
        if ctx is not None:
            ctx.close()
