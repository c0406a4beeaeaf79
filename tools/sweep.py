#!/usr/bin/env python3
"""Pigment sweep: render one scene once per row of a csv with columns H, M, E, B (blood, melanin,
epidermis thickness x 1e6 nm, eumelanin fraction; the fork's utilities/python/SceneMaker.py over
utilities/csv/perms.csv), writing one image per row.

  --mode update   one context; per row the material is rebuilt in place (mpss_update_layeredskin),
                  Preprocess reuses its surface points, the scene buffers stay on the device
  --mode fresh    a new context per row (the only way without mpss_update_layeredskin): the comparison
  --spectral      every row also renders its 30-band radiance cube (mpss_render_tiles_spectral, one call for
                  both films) and writes it as perm_NNNN_spectral.exr: apply your own illuminant and sensor
                  curves to the band radiances instead of the CIE observer baked into the image

Prints one JSON line per permutation (seconds of the material build, Preprocess, render and image
write) and a summary line (permutations/s over the whole run; median, min and max of each stage).
--split adds, per row, the material build's parts from host timers around existing calls:
tables_s = the same tables installed with mpss_set_material_tables on a scratch context (device
copies + the two common grids, no profile or rho build), grid_s = the two common grids alone
(mpss_host_common_grid for both LDS layouts on two threads, as the build runs them), so
profile_rho_s = material_s - tables_s and upload_s = tables_s - grid_s. The split is indirect: the
work is redone beside the build, not timed inside it, and upload_s is a difference of two such
timings (it scatters by the timings' own spread).
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v2-skin_amd"))
DEFAULT_CSV = os.path.join(ROOT, "tests", "golden", "perms_first16.csv")


def split_material(mpss, ctx, mid, material_s):
    tab, rcp, rho, _ = ctx.material_tables(mid)
    cfg = {k: getattr(ctx.cfg, k) for k, _ in mpss.Config._fields_}
    scratch = mpss.Context(**cfg)
    try:
        t0 = time.perf_counter()
        scratch.set_material_tables(tab, rcp, rho)
        tables_s = time.perf_counter() - t0
    finally:
        scratch.close()

    def grid(nf):  # (sizes first, then the rows: two builds per call)
        mpss.host_common_grid(tab, rcp, snake=bool(ctx.cfg.mo_band_dealing), near_field=nf)
    th = [threading.Thread(target=grid, args=(nf,)) for nf in (10236, 5088)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    grid_s = (time.perf_counter() - t0) / 2
    return dict(tables_s=tables_s, grid_s=grid_s, profile_rho_s=max(0.0, material_s - tables_s),
                upload_s=max(0.0, tables_s - grid_s))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("scene", help="a .pbrt scene with a layeredskin material (e.g. scenes/skin.pbrt)")
    ap.add_argument("csv", nargs="?", default=DEFAULT_CSV, help="pigment csv with H, M, E, B columns "
                    "(default: tests/golden/perms_first16.csv)")
    ap.add_argument("--out", default="sweep_out", metavar="DIR", help="directory for the images")
    ap.add_argument("--limit", type=int, default=None, metavar="N", help="render only the first N rows")
    ap.add_argument("--mode", choices=("update", "fresh"), default="update")
    ap.add_argument("--format", choices=("pfm", "exr"), default="exr")
    ap.add_argument("--material", type=int, default=0, help="index of the material the pigments apply to")
    ap.add_argument("--grid-builder", choices=("host", "gpu"), default=None,
                    help="the common-grid builder of the material builds (default: the library's)")
    ap.add_argument("--split", action="store_true", help="split the material build (extra work per row)")
    ap.add_argument("--no-write", action="store_true", help="skip the image files (timing runs)")
    ap.add_argument("--spectral", action="store_true", help="also render the 30-band radiance cube of every row "
                    "and write it beside the image as perm_NNNN_spectral.exr (30 FLOAT channels S0.<centre>nm)")
    args = ap.parse_args(argv)

    import mpss
    from mpss import film, pbrtscene
    from mpss import sweep as sw

    rows = sw.read_rows(args.csv, args.limit)
    if not rows:
        raise SystemExit("no complete H, M, E, B rows in %s" % args.csv)
    sc = pbrtscene.load(args.scene)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
    per_stage = {}
    t_run = time.perf_counter()
    t_row = t_run
    for i, (xyzw, secs, ctx) in enumerate(sw.sweep(sc, rows, mode=args.mode, material=args.material,
                                                    grid_on_host=None if args.grid_builder is None else
                                                    args.grid_builder == "host", spectral=args.spectral)):
        t0 = time.perf_counter()
        spec = None
        if args.spectral:
            xyzw, spec = xyzw
        if not args.no_write:
            film.write_image(os.path.join(args.out, "perm_%04d.%s" % (i, args.format)), film.finalize(xyzw))
            if spec is not None:
                film.write_spectral_exr(os.path.join(args.out, "perm_%04d_spectral.exr" % i),
                                        film.finalize_spectral(spec))
        secs["write_s"] = time.perf_counter() - t0
        secs["total_s"] = time.perf_counter() - t_row
        if args.split:
            secs.update(split_material(mpss, ctx, args.material, secs["material_s"]))
        line = dict(perm=i, mode=args.mode, H=rows[i][0], M=rows[i][1], E=rows[i][2], B=rows[i][3])
        line.update({k: round(v, 6) for k, v in secs.items()})
        print(json.dumps(line), flush=True)
        for k, v in secs.items():
            per_stage.setdefault(k, []).append(v)
        t_row = time.perf_counter()
    wall = time.perf_counter() - t_run
    summary = dict(summary=True, mode=args.mode, grid_builder=args.grid_builder or "default", scene=os.path.basename(args.scene), permutations=len(rows),
                   wall_s=round(wall, 6), perms_per_s=round(len(rows) / wall, 6))
    for k, v in per_stage.items():
        summary[k] = dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6))
    print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
