#!/usr/bin/env python
"""Time the batched profile fit: a 5 x 2 x 5 x 3 grid (150 combinations, 4500 profiles) at desiredProfileLength
256 through mpss_profile_fit, seconds per combination, with the profile stage and the fit stage separated by HIP
events. The comparison is the only other route to the same profiles: one mpss_add_layeredskin per combination
at desired_length 256 with mo_common_grid 0 -- which also builds a rho table, and copies its table back, that
the fit does not need. Both are timed in this process, after one warm-up each; the median of --repeats runs.

    python tools/bench_profilefit.py [--repeats 3]
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v2-skin_amd"))

GRID = dict(f_mel=[0.01, 0.03, 0.08, 0.15, 0.3], f_eu=[0.3, 0.7], f_blood=[0.002, 0.01, 0.02, 0.05, 0.1],
            f_ohg=[0.3, 0.6, 0.9])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--desired-length", type=int, default=256)
    a = ap.parse_args()
    import torch
    import mpss
    ctx = mpss.Context(mo_common_grid=0)
    fit = mpss.profile_fit_spec(desired_length=a.desired_length, **GRID)
    n = 5 * 2 * 5 * 3
    ctx.profile_fit(mpss.profile_fit_spec(desired_length=a.desired_length, id_range=(0, 4), **GRID))  # warm-up
    wall, prof, fitms = [], [], []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = ctx.profile_fit(fit, timing=True)
        wall.append(time.perf_counter() - t)
        prof.append(r["stage_ms"][0] * 1e-3)
        fitms.append(r["stage_ms"][1] * 1e-3)
    combos = [(m, e, b, o) for m in GRID["f_mel"] for e in GRID["f_eu"] for b in GRID["f_blood"] for o in GRID["f_ohg"]]
    mk = lambda c: mpss.default_skin(desired_length=a.desired_length, nmperunit=1e6, f_mel=c[0], f_eu=c[1],
                                     f_blood=c[2], f_ohg=c[3])
    ctx.close()
    base = []
    for _ in range(a.repeats):  # a context holds at most 256 materials: a fresh one per repeat, warmed up
        ctx = mpss.Context(mo_common_grid=0)
        ctx.add_layeredskin(mk(combos[0]))
        torch.cuda.synchronize()
        t = time.perf_counter()
        for c in combos:
            ctx.add_layeredskin(mk(c))
        torch.cuda.synchronize()
        base.append((time.perf_counter() - t) / len(combos))
        ctx.close()
    med = statistics.median
    print(json.dumps(dict(
        combinations=n, desired_length=a.desired_length, repeats=a.repeats,
        batched_s_per_combination=med(wall) / n, profile_stage_s_per_combination=med(prof) / n,
        fit_stage_s_per_combination=med(fitms) / n, batched_wall_s=wall,
        baseline_s_per_combination=med(base), baseline_combinations=len(combos), baseline_runs=base,
        baseline_note="one mpss_add_layeredskin per combination: 30-band profile at desired_length %d, "
                      "mo_common_grid 0; it also builds a rho table"
                      % a.desired_length)))


if __name__ == "__main__":
    main()
