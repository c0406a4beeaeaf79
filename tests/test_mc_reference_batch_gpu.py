"""The batched multipole references on the GPU (mpss_mc_reference_batch, profile_gpu.hip) against the oracle's
MPC (kissfft transforms): MultipoleReferenceTask::Run (renderers/mcprofile.cpp:381-425) per slab.

Tolerances are the project's bound for GPU-built profiles (test_c2_tables_at_desired_length_512,
test_usemontecarlo_tables_vs_oracle): 1e-6 of the oracle's peak per ring, 1e-6 relative for the totals. Ring 0
is held to 1e-6 relative on its own and left out of the peak: with the lerp on, T's ring 0 carries the thin
slab's delta and would set it."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import oracle_mc

pytestmark = pytest.mark.gpu
C4_LAYERS = [(723.6646118164062, 577.9549560546875, 1.399999976158142, 0.0024999999441206455),
             (9.664658546447754, 288.97747802734375, 1.399999976158142, 0.20000000298023224)]
TOPS = (1e-5, 4e-4, 1.2e-3, 2.5e-3, 1e-2)  # the top layer's 2 mfp is 1.54e-3: three thin slabs, two thick


def c4_slabs(tops):
    lay = np.repeat(np.asarray(C4_LAYERS, np.float32)[None], len(tops), axis=0)
    lay[:, 0, 3] = tops
    return lay


@pytest.fixture(scope="module")
def ctx(mpss, oracle):
    import torch
    assert torch.cuda.is_available()
    return mpss.Context()


def oracle_reference(layers, mfp_range, nseg, lerp, length):
    """oracle_mc.mc_reference at another desired length."""
    lay = np.asarray(layers, np.float32).reshape(-1, 4)
    mfp = sum(1.0 / float(np.float32(a + b)) for a, b in lay[:, :2])
    extent = float(np.float32(mfp_range)) * (mfp / len(lay))
    specs = [(float(l[2]), float(l[3]), float(l[0]), float(l[1])) for l in lay]
    d, r, t, tr, tt = oracle_lib.mpc_profile(specs, float(np.float32(extent * 1.01 / length)), length, lerp, False)
    L = oracle_lib.lib()
    L.o_mpc_resample.argtypes = [C.c_int] + [oracle_lib.f32p] * 3 + [C.c_int] + [oracle_lib.f32p] * 3
    pts = ((np.arange(nseg) + 0.5) * (extent / nseg)).astype(np.float32)
    ro, to = np.zeros(nseg, np.float32), np.zeros(nseg, np.float32)
    L.o_mpc_resample(len(d), d, r, t, nseg, pts, ro, to)
    return dict(reflectance=ro.astype(np.float64), transmittance=to.astype(np.float64), total_r=tr, total_t=tt)


def compare(got, s, ref, tag):
    for k in ("reflectance", "transmittance"):
        g, o = got[k][s], ref[k]
        peak = np.abs(o[1:]).max()
        err = np.abs(g[1:] - o[1:]).max() / peak
        e0 = abs(g[0] - o[0]) / abs(o[0])
        print(tag, s, k, "rings 1.. %.3g of peak, ring 0 %.3g relative" % (err, e0))
        assert err <= 1e-6, (tag, s, k, err)
        assert e0 <= 1e-6, (tag, s, k, e0)
    for k in ("total_r", "total_t"):
        print(tag, s, k, got[k][s] / ref[k] - 1.0)
        assert got[k][s] == pytest.approx(ref[k], rel=1e-6), (tag, s, k)


@pytest.mark.parametrize("length", [64, 128])
def test_small_grids_vs_oracle(ctx, length):
    lay = c4_slabs(TOPS)
    got = {lerp: ctx.mc_reference_batch(lay, 16.0, 32, lerp, desired_length=length) for lerp in (False, True)}
    for lerp in (False, True):
        for s in range(len(lay)):
            compare(got[lerp], s, oracle_reference(lay[s], 16.0, 32, lerp, length), "L%d lerp%d" % (length, lerp))
    for s in range(len(lay)):  # the flag reaches the kernels: it matters below 2 mfp only
        same = all(np.array_equal(got[False][k][s], got[True][k][s])
                   for k in ("reflectance", "transmittance", "total_r", "total_t"))
        assert same == (s >= 3), (s, same)
        if s < 3:
            assert got[False]["total_t"][s] != got[True]["total_t"][s]


def test_batch_limit_does_not_change_results(ctx):
    lay = c4_slabs(TOPS)
    a = ctx.mc_reference_batch(lay, 16.0, 32, True, desired_length=64, max_profiles_per_batch=1)
    b = ctx.mc_reference_batch(lay, 16.0, 32, True, desired_length=64, max_profiles_per_batch=0)
    c = ctx.mc_reference_batch(lay, 16.0, 32, True, desired_length=64, max_profiles_per_batch=2)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(c[k], b[k]), k


def test_full_size_vs_oracle(ctx):
    got = ctx.mc_reference_batch(c4_slabs(TOPS[3:4]), 16.0, 256, True)  # desired_length 1024: M = 4096
    compare(got, 0, oracle_mc.mc_reference(C4_LAYERS, 16.0, 256, True), "L1024")


def test_other_layer_counts_take_the_host_path(ctx, mpss):
    one = np.asarray([[(0.05, 1.0, 1.4, 50.0)], [(0.2, 2.0, 1.33, 30.0)]], np.float32)
    got = ctx.mc_reference_batch(one, 16.0, 32, True)
    for s in range(2):
        ref = mpss.mc_reference(one[s], 16.0, 32, True)
        for k in ref:
            assert np.array_equal(got[k][s], ref[k]), (s, k)


def test_validation(ctx, mpss):
    with pytest.raises(mpss.MpssError, match="desired length"):
        ctx.mc_reference_batch(c4_slabs(TOPS[:2]), 16.0, 32, True, desired_length=2048)
    bad = c4_slabs(TOPS[:3])
    bad[1, 0, 3] = 0.0
    with pytest.raises(mpss.MpssError, match="thickness > 0"):
        ctx.mc_reference_batch(bad, 16.0, 32, True, desired_length=64)
