#!/usr/bin/env python3
"""What the spectral film costs on the C2 frame (skin.pbrt 1024 x 1024 at 64 spp, 128-pixel tiles, one GPU): the
frame's wall time and the film step's kernel time (mpss_get_render_stats with kernel_timing: assemble + sky + the
film kernels) for the XYZ frame (mpss_render_tiles), the spectral frame with its XYZW film beside the cube, and
the spectral frame alone (mpss_render_tiles_spectral with and without xyzw_dev). Prints one JSON line per
variant. frame_ms is the mean of the timed frames; ms_film comes from one further frame of its own with
kernel_timing on (the timing events serialise the steps), not from the timed frames. No pass mark.

    python tools/bench_spectral.py [--res 1024] [--spp 64] [--tile 128] [--steps 3] [--warmup 1] [--filter box]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v2-skin_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "skin.pbrt"))
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--filter", default="box", help="box (0.5 / 0.5, the default) or another kind at its own widths")
    a = ap.parse_args()
    import torch
    from mpss import pbrtscene, tiles as tl
    sc = pbrtscene.load(a.scene, xres=a.res, yres=a.res, spp=a.spp)
    ctx = pbrtscene.build_context(sc)
    ctx.preprocess(seed=1)
    ctx.set_pixel_filter(a.filter)
    rects = tl.tile_grid(sc.xres, sc.yres, a.tile)
    outs = [torch.zeros(((y1 - y0) * (x1 - x0) * 4,), dtype=torch.float32, device="cuda") for x0, x1, y0, y1 in rects]
    cube = [torch.zeros(((y1 - y0) * (x1 - x0) * 32,), dtype=torch.float32, device="cuda") for x0, x1, y0, y1 in rects]
    ptrs, sptrs = [o.data_ptr() for o in outs], [c.data_ptr() for c in cube]
    variants = (("xyz", lambda: ctx.render_tiles(a.spp, a.seed, rects, ptrs)),
                ("spectral+xyz", lambda: ctx.render_tiles_spectral(a.spp, a.seed, rects, sptrs, ptrs)),
                ("spectral", lambda: ctx.render_tiles_spectral(a.spp, a.seed, rects, sptrs)))
    for name, frame in variants:
        ctx.set_instrumentation(kernel_timing=False)
        for _ in range(a.warmup):
            frame()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            frame()
        torch.cuda.synchronize()
        frame_ms = (time.perf_counter() - t0) * 1e3 / a.steps
        # kernel times from a pass of their own (the events serialise the steps)
        ctx.set_instrumentation(kernel_timing=True)
        ctx.reset_render_stats()
        frame()
        torch.cuda.synchronize()
        st = ctx.render_stats()
        print(json.dumps({"variant": name, "filter": a.filter, "res": a.res, "spp": a.spp, "tile": a.tile,
                          "frame_ms": round(frame_ms, 2), "samples_traced": st["samples"],
                          "ms_film": round(st["ms_film"], 3), "n_film": st["n_film"]}), flush=True)


if __name__ == "__main__":
    main()
