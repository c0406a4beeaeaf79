#!/usr/bin/env python
"""Run a Renderer "batchmcprofile" scene: sweep the top layer's thickness, trace every thickness's photons in one
batched walk, compute the multipole references (lerp off and on) on the GPU, and write the reference's table.

    python tools/batchmcprofile.py scenes/batchmcprofile.pbrt [--photons N] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v2-skin_amd"))


def run(scene, photons=None, out=None, device=0):
    """The scene's renderer, rendered; (renderer, table path)."""
    import mpss
    from mpss import batchmcprofile, pbrtscene
    sc = pbrtscene.load(scene)
    if not sc.renderer or sc.renderer[0] != "batchmcprofile":
        raise ValueError("%s does not select Renderer \"batchmcprofile\"" % scene)
    r = batchmcprofile.create_from_params(sc.renderer[1])
    if photons is not None:
        r.photons = int(photons)
    path = out or r.filename
    if path and not os.path.isabs(path) and not out:  # FindOneFilename: relative to the scene file
        path = os.path.join(os.path.dirname(os.path.abspath(scene)), path)
    r.filename = path
    ctx = mpss.Context(device=device)
    try:
        r.render(ctx)
    finally:
        ctx.close()
    return r, path


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("scene")
    ap.add_argument("--photons", type=int, help="photons per thickness (default: the scene's \"photons\")")
    ap.add_argument("--out", help="table file (default: the scene's \"filename\")")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    t = time.perf_counter()
    try:
        r, path = run(a.scene, a.photons, a.out, a.device)
    except ValueError as e:
        sys.exit(str(e))
    print("%d thicknesses x %d photons, %d events, %.2f s" % (len(r.results), r.photons, r.events,
                                                               time.perf_counter() - t))
    if path:
        print("wrote %s" % path)


if __name__ == "__main__":
    main()
