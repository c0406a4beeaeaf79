#!/usr/bin/env python
"""Run a Renderer "multipoleprofilefit" scene: fit sums of Gaussians to the skin profiles of its parameter grid
and write the reference's text table.

    python tools/profilefit.py scenes/profilefit.pbrt [--host] [--out FILE] [--idrange A B]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v2-skin_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("scene")
    ap.add_argument("--host", action="store_true", help="the host restatement instead of the GPU")
    ap.add_argument("--out", help="table file (default: the scene's \"filename\")")
    ap.add_argument("--idrange", type=int, nargs=2, help="overrides the scene's \"idrange\"")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import mpss
    from mpss import pbrtscene, profilefit
    sc = pbrtscene.load(a.scene)
    if not sc.renderer or sc.renderer[0] != "multipoleprofilefit":
        sys.exit("%s does not select Renderer \"multipoleprofilefit\"" % a.scene)
    d = sc.renderer[1]
    id_range = tuple(a.idrange) if a.idrange else d["id_range"]
    ctx = None if a.host else mpss.Context(device=a.device)
    res, id_min = profilefit.run(d["ranges"], d["layers"], d["desired_length"], id_range, ctx=ctx, timing=ctx is not None)
    if ctx is not None:
        print("profiles %.1f ms, fit %.1f ms for %d ids" % (res["stage_ms"] + (len(res["coeffs"]),)))
        ctx.close()
    out = a.out or d["filename"]
    if out and len(res["coeffs"]):
        with open(out, "w", newline="\n") as f:
            profilefit.write_table(f, d["ranges"], res, id_min)
        print("wrote %s" % out)
    worst = float(res["error"].max()) if len(res["coeffs"]) else 0.0
    print("%d ids, %d sigmas, largest fit error %.2f%%" % (len(res["coeffs"]), len(res["sigmas"]), 100 * worst))


if __name__ == "__main__":
    main()
