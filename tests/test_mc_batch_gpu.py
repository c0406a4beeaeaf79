"""The batched walk (mpss_mc_profile_batch, mc_profile_batch.hip) against the single-slab walk and the oracle.

A slab in a batch walks the photon streams (seed, k) through the single kernel's own step, so its tallies hold
the same terms as ctx.mc_profile's in another order: totals and ring sums (photon fractions) agree within 1e-9
absolute -- test_energy_conservation's bound; the derived one, n * 2^-53 for n weights of at most 1, is far
below it. Against the oracle the comparison is statistical, by test_matches_oracle's criteria."""
import numpy as np
import pytest

import oracle_mc

pytestmark = pytest.mark.gpu
C4_LAYERS = [(723.6646118164062, 577.9549560546875, 1.399999976158142, 0.0024999999441206455),
             (9.664658546447754, 288.97747802734375, 1.399999976158142, 0.20000000298023224)]
TOPS = (1e-5, 4e-4, 1.2e-3, 2.5e-3, 1e-2)


def c4_slabs(tops):
    lay = np.repeat(np.asarray(C4_LAYERS, np.float32)[None], len(tops), axis=0)
    lay[:, 0, 3] = tops
    return lay


@pytest.fixture(scope="module")
def ctx(mpss):
    import torch
    assert torch.cuda.is_available()
    return mpss.Context()


def ring_area(extent, nseg):
    i = np.arange(nseg, dtype=np.float64)
    return oracle_mc.PBRT_PI * ((2 * i + 1) * extent / nseg) * (extent / nseg)


def check_against_single(ctx, lay, nseg, n, seed=89, mfp_range=16.0):
    """Every slab of the rings call and of the totals-only call against its own ctx.mc_profile."""
    b = ctx.mc_profile_batch(lay, mfp_range, nseg, n, seed=seed)
    t = ctx.mc_profile_batch(lay, mfp_range, nseg, n, seed=seed, rings=False)
    assert t["reflectance"] is None and t["transmittance"] is None
    assert b["reflectance"].shape == (len(lay), nseg) and b["total_r"].shape == (len(lay),)
    ev = 0
    for s in range(len(lay)):
        one = ctx.mc_profile(lay[s], mfp_range, nseg, n, seed=seed)
        ev += one["events"]
        area = ring_area(b["extent"][s], nseg)
        for k in ("total_r", "total_t"):
            print(s, k, b[k][s] - one[k], t[k][s] - one[k])
            assert abs(b[k][s] - one[k]) <= 1e-9, (s, k, b[k][s], one[k])
            assert abs(t[k][s] - one[k]) <= 1e-9, (s, k, t[k][s], one[k])
        for k in ("reflectance", "transmittance"):
            assert np.all(np.abs(b[k][s] * area - one[k] * area) <= 1e-9), (s, k)
    assert b["events"] == ev and t["events"] == ev  # the same walks, event for event
    return b


def test_batch_equals_single(ctx):
    b = check_against_single(ctx, c4_slabs(TOPS), 64, 20_000)
    assert len(set(np.round(b["total_r"], 6))) == len(TOPS)  # five different slabs
    assert np.all(np.diff(b["extent"]) == 0)  # the extent does not depend on the thickness


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_photon_counts_around_a_pool(ctx, n):
    check_against_single(ctx, c4_slabs(TOPS[1:4]), 64, n)


def test_one_slab(ctx):
    check_against_single(ctx, c4_slabs(TOPS[3:4]), 64, 20_000)


def test_more_slabs_than_lanes(ctx):
    check_against_single(ctx, c4_slabs(np.linspace(1e-5, 5e-3, 70)), 8, 300)


def test_one_and_three_layers(ctx):
    one = np.asarray([[(0.01, 1.0, 1.4, 50.0)], [(0.05, 2.0, 1.33, 3.0)]], np.float32)
    check_against_single(ctx, one, 64, 5000)
    three = np.asarray([[(0.2, 3.0, 1.4, 0.25), (0.05, 1.5, 1.4, 5.0), (0.1, 1.0, 1.3, 2.0)],
                        [(0.2, 3.0, 1.4, 0.05), (0.05, 1.5, 1.45, 1.0), (0.1, 1.0, 1.3, 2.0)]], np.float32)
    check_against_single(ctx, three, 64, 5000)


def test_energy_conservation(ctx):
    lay = np.asarray([[(0.0, 2.0, 1.4, t), (0.0, 0.5, 1.3, 2.0)] for t in (0.01, 0.1, 0.3, 1.0)], np.float32)
    for rings in (True, False):
        o = ctx.mc_profile_batch(lay, 2000, 64, 50000, seed=3, rings=rings)
        print(rings, o["total_r"] + o["total_t"] - 1.0)
        assert np.all(np.abs(o["total_r"] + o["total_t"] - 1.0) <= 1e-9)
        assert o["events"] > 4 * 50000


def test_matches_oracle(ctx):
    n, nseg = 200000, 1024
    lay = c4_slabs((4e-4, 2.5e-3, 1e-2))
    g = ctx.mc_profile_batch(lay, 16, nseg, n, seed=89)
    for s in range(len(lay)):
        c = oracle_mc.mc_profile(lay[s], mfp_range=16, nsegments=nseg, nphotons=n, seed=89)
        assert g["extent"][s] == pytest.approx(c["extent"], rel=1e-14)
        for k in ("total_r", "total_t"):
            p = max(c[k], 1.0 / n)
            sigma = np.sqrt(p * (1 - min(p, 0.999)) / n)
            assert abs(g[k][s] - c[k]) <= 4 * sigma + 1e-12, (s, k, g[k][s], c[k])
        area = ring_area(c["extent"], nseg)
        gr = (g["reflectance"][s] * area).reshape(16, 64).sum(1)
        cr = (c["reflectance"] * area).reshape(16, 64).sum(1)
        sig = np.sqrt(np.maximum(cr, 1.0 / n) / n)
        assert np.all(np.abs(gr - cr) <= 5 * sig), (s, np.abs(gr - cr) / sig)


def test_validation(ctx, mpss):
    lay = c4_slabs(TOPS[:3])
    lay[2, 1, 1] = 0.0  # musp = 0 in the last slab
    with pytest.raises(mpss.MpssError, match="musp > 0"):
        ctx.mc_profile_batch(lay, nphotons=10)
    with pytest.raises(mpss.MpssError, match="segments"):
        ctx.mc_profile_batch(c4_slabs(TOPS[:3]), nsegments=0, nphotons=10)
    z = ctx.mc_profile_batch(c4_slabs(TOPS[:3]), nsegments=8, nphotons=0)
    assert not z["total_r"].any() and not z["reflectance"].any() and z["events"] == 0
