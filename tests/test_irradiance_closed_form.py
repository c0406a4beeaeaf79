"""The oracle's point irradiance under one sphere light against a reference that is not a
restatement of the reference's code (CPU only): the solid angle of the disc a point sees.

An unoccluded point without a BSSRDF sees the whole sphere above its horizon. Sphere::Sample draws
directions uniformly in the cone of half-angle alpha = asin(R/d), so every term of IrradianceTask's
estimator is L Omega cos(theta_i) and E is bracketed by the extreme cosines over the cone
(irradiance_hostile.closed_form). A pdf constant wrong in both the product and the oracle would pass
the parity tests; it cannot pass this. The GPU's values meet the same bracket in
tests/test_irradiance_hostile_gpu.py.

The last test pins the three regimes of the distance ladder as the reference's float arithmetic
produces them (UniformConePdf's 1 - cosThetaMax, montecarlo.cpp:409-411): the closed form while 1 -
ctmax keeps its digits, a wrong but positive E once it has lost them (R/d = 1e-3: 1 - ctmax is one
of 8 or 9 ulps of 1), and exactly 0 once ctmax rounds to 1 (pdf = +inf, every term x / inf).
"""
import numpy as np
import pytest

import irradiance_hostile as ih
import oracle_render as orr


@pytest.fixture(scope="module")
def osc(oracle):
    import mpss
    from mpss import pbrtscene
    sc = ih.scene([ih.sphere_light(64)])
    cfg = mpss.default_config(**pbrtscene.integrator_config(sc))
    o = orr.OracleScene(sc, ih.irradiance_tables(sc), cfg, mpss)
    yield o
    o.close()


def test_oracle_irradiance_within_the_closed_form_bracket(osc):
    E = osc.irradiance(ih.closed_form_points(), 7, nthreads=8)
    ih.check_closed_form(E)


def test_ladder_regimes_of_the_oracle(osc):
    pts, meta = ih.ladder_points()
    E = osc.irradiance(pts, 7, nthreads=8)
    assert np.all(np.isfinite(E))
    L = ih.lemit_bands()
    facing = {rd: E[i].astype(np.float64) for i, (rd, j) in enumerate(meta) if j == 0}
    for i, (rd, j) in enumerate(meta):
        if j == 2:  # the normal faces away: nothing arrives
            assert np.all(E[i] == 0), rd
    for rd in (0.5, 0.1, 0.01):
        lo, hi, _ = ih.closed_form(rd, 0.0, L)
        assert np.all(facing[rd] >= lo) and np.all(facing[rd] <= hi), rd
    lo, hi, _ = ih.closed_form(1e-3, 0.0, L, rounding=False)   # what exact arithmetic would allow
    e = facing[1e-3]
    assert np.all(e > 0) and (np.all(e < lo) or np.all(e > hi)), (e / lo, e / hi)
    for rd in (1e-4, 1e-5):
        assert np.all(facing[rd] == 0), rd
