#!/usr/bin/env python
"""Time the two halves of Renderer "batchmcprofile" on scenes/batchmcprofile.pbrt's slabs (257 thicknesses of the
top layer), each against the only other route to the same numbers, in this process:

(a) the walk: one mpss_mc_profile_batch call (totals only) against a loop of one ctx.mc_profile per slab, at
    --photons per slab. One warm-up of each, then --repeats timed runs of each, interleaved; the median and the
    spread (min .. max) of both are reported. Wall-clock around calls that are synchronous on their stream.
(b) the multipole references: the two mpss_mc_reference_batch calls (lerp off and on, 2 x 257 profiles at
    desiredLength 1024) against the host mpss.mc_reference on --host-slabs slabs spread over the sweep, reported
    per profile (the host is not run on all 514).

    python tools/bench_batchmc.py [--repeats 5] [--photons 1000000] [--skip-b]
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


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--photons", type=int, default=None, help="per slab (default: the scene's)")
    ap.add_argument("--ref-repeats", type=int, default=2)
    ap.add_argument("--host-slabs", type=int, default=4)
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    import torch
    import mpss
    from mpss import batchmcprofile, pbrtscene
    sc = pbrtscene.load(os.path.join(ROOT, "scenes", "batchmcprofile.pbrt"))
    r = batchmcprofile.create_from_params(sc.renderer[1])
    n = a.photons or r.photons
    lay = r.slabs()
    S = len(lay)
    ctx = mpss.Context()

    def batched():
        torch.cuda.synchronize()
        t = time.perf_counter()
        o = ctx.mc_profile_batch(lay, r.mfp_range, r.segments, n, seed=r.seed, rings=False)
        return time.perf_counter() - t, o

    def looped():
        torch.cuda.synchronize()
        t = time.perf_counter()
        o = [ctx.mc_profile(lay[s], r.mfp_range, r.segments, n, seed=r.seed) for s in range(S)]
        return time.perf_counter() - t, o

    _, ob = batched()  # warm-up of each
    _, ol = looped()
    worst = max(max(abs(ob["total_r"][s] - ol[s]["total_r"]), abs(ob["total_t"][s] - ol[s]["total_t"]))
                for s in range(S))
    tb, tl = [], []
    for _ in range(a.repeats):
        tb.append(batched()[0])
        tl.append(looped()[0])
    out = dict(slabs=S, photons_per_slab=n, segments=r.segments, repeats=a.repeats, events=ob["events"],
               walk_batched_s=stats(tb), walk_loop_s=stats(tl),
               walk_batched_photons_per_s=S * n / statistics.median(tb),
               walk_loop_photons_per_s=S * n / statistics.median(tl),
               walk_loop_spread_s=max(tl) - min(tl),
               walk_batched_minus_loop_s=statistics.median(tb) - statistics.median(tl),
               walk_largest_total_difference=worst)
    if not a.skip_b:
        def refs():
            torch.cuda.synchronize()
            t = time.perf_counter()
            o = [ctx.mc_reference_batch(lay, r.mfp_range, r.segments, lerp) for lerp in (False, True)]
            return time.perf_counter() - t, o
        _, og = refs()
        tg = [refs()[0] for _ in range(a.ref_repeats)]
        pick = [round(i * (S - 1) / max(1, a.host_slabs - 1)) for i in range(a.host_slabs)]
        th, dev = [], 0.0
        for s in pick:
            t = time.perf_counter()
            h = mpss.mc_reference(lay[s], r.mfp_range, r.segments, True)
            th.append(time.perf_counter() - t)
            dev = max(dev, abs(og[1]["total_r"][s] / h["total_r"] - 1.0), abs(og[1]["total_t"][s] / h["total_t"] - 1.0))
        out.update(reference_profiles=2 * S, reference_gpu_s=stats(tg),
                   reference_gpu_s_per_profile=statistics.median(tg) / (2 * S),
                   reference_host_slabs=pick, reference_host_s_per_profile=stats(th),
                   reference_host_threads=min(16, os.cpu_count() or 1),
                   reference_largest_relative_total_difference=dev)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
