"""mpss_profile_fit end to end on the GPU: batched FP64 profiles (csrc/profile_gpu.hip) feeding the fit kernel
(csrc/sog_fit.hip), for sog_ref.GRID (2 x 1 x 2 x 2: 8 ids, 240 profiles) at desiredProfileLength 16 and 64.

Against the host (mpss_host_profile_fit: host FFT profiles + the host fit) the coefficients of ill-conditioned
windows are no fair measure, so two things are compared per (id, band):
  * error[id][band] (overallError), absolute difference;
  * the fitted curve, evaluated in float64 from the returned coefficients, in the error term's own weighted
    norm: sqrt(sum r (fit_a - fit_b)^2 dr / sum r y^2 dr).
The allowance for each is 8 x the spread the host fit itself shows between two reference-grade profiles of the
same layers -- the library's host build and the oracle's kissfft build -- over the 60 profiles of ids 0 and 5.
At desiredProfileLength 16 the two reference profiles are the same floats (spread 0), and 8 x 0 would ask the
GPU for bit identity, which differently ordered FP64 transforms and sums cannot give. So each allowance has a
floor from the number formats, FLOOR below:
  * the profiles are floats taken from FP64 grids that agree to FP64 rounding, so a sample may differ by one
    float ulp, and by one more through the float lerp of the resampling: |dy| <= 2 * 2^-23 |y| = 2^-22 |y|
    pointwise, hence ||dy|| <= 2^-22 ||y|| in the weighted norm;
  * the fitted curve is a least-squares projection of y, taken as non-expansive: the curve moves by at most
    ||dy|| / ||y|| <= 2^-22, and the residual by that plus dy itself, so the error by at most 2 * 2^-22;
  * both sides return floats: one float ulp of the result on top (2^-23 of the error; 2^-23 of the summed
    weighted norms of the six terms, each coefficient being one float rounding).
Measured on the GPU (both lengths: the two reference profiles are the same floats, so the floor is the
allowance): error difference 1.2e-8 at 16 and 3.4e-8 at 64 (0.03 and 0.07 of the allowance), curve difference
2.1e-7 and 2.2e-7 (0.57 and 0.60 of it). The figures are printed by the test; BASELINE.md section 3 records them.
"""
import numpy as np
import pytest

import sog_ref

pytestmark = pytest.mark.gpu

DESIRED = (16, 64)
FLOOR = 2.0 ** -22  # two float ulps of the profile samples (module docstring)


@pytest.fixture(scope="module")
def ctx(mpss):
    c = mpss.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def full(mpss, ctx):
    out = {dl: ctx.profile_fit(mpss.profile_fit_spec(desired_length=dl, **sog_ref.GRID), timing=True) for dl in DESIRED}
    assert all(r["batches"] == 1 for r in out.values())  # 240 profiles fit one batch
    return out


def _curve_distance(sig, r, y, row_a, row_b):
    return sog_ref.curve_distance(sig, r, y, row_a, row_b)


def _term_norms(sig, r, y, row):
    return sog_ref.term_norms(sig, row, r, y)


def _spread(mpss, oracle, case, dl):
    """the host fit on the library's host profile against the host fit on the oracle's profile, ids 0 and 5"""
    sig = case["host"]["sigmas"]
    d_err = d_curve = 0.0
    for i in (0, 5):
        mua, musp, th, eta = mpss.profilefit_layers(case["fit"], i)
        for b in range(30):
            p = i * 30 + b
            layers = [(mua[l, b], musp[l, b], eta[l], th[l]) for l in range(2)]
            d, y = sog_ref.oracle_fit_profile(oracle, layers, dl)
            o = mpss.host_sog_fit(d, y, sig, case["mfp_min"][p], case["mfp_max"][p])
            r = np.sqrt(case["dist_sq"][p]).astype(np.float64)
            d_err = max(d_err, abs(float(o["error"][0]) - float(case["sog"]["error"][p])))
            d_curve = max(d_curve, _curve_distance(sig, r, case["data"][p], o["coeffs"][0], case["sog"]["coeffs"][p]))
    return d_err, d_curve


@pytest.mark.parametrize("dl", DESIRED)
def test_batch_split_changes_no_bit(mpss, ctx, full, dl):
    split = ctx.profile_fit(mpss.profile_fit_spec(desired_length=dl, max_profiles_per_batch=100, **sog_ref.GRID),
                            timing=True)
    assert split["batches"] == 3  # the cap was honoured: the folded inverse transform ran on 100, 100 and 40 channels
    for k in ("sigmas", "coeffs", "error", "rgb_coeffs", "centre"):  # batches of 100, 100 and 40 profiles
        assert split[k].tobytes() == full[dl][k].tobytes(), k


@pytest.mark.parametrize("dl", DESIRED)
def test_against_host_profiles_and_host_fit(mpss, oracle, full, dl):
    case = sog_ref.grid_case(mpss, dl)
    host, gpu = case["host"], full[dl]
    assert np.array_equal(gpu["sigmas"], host["sigmas"])
    s_err, s_curve = _spread(mpss, oracle, case, dl)
    print("desired %d: host-profile vs oracle-profile spread: error %.3e, curve %.3e" % (dl, s_err, s_curve))
    w_err = w_curve = 0.0  # worst difference over its allowance
    m_err = m_curve = 0.0
    for i in range(8):
        for b in range(30):
            p = i * 30 + b
            r = np.sqrt(case["dist_sq"][p]).astype(np.float64)
            d_err = abs(float(gpu["error"][i, b]) - float(host["error"][i, b]))
            d_curve = _curve_distance(host["sigmas"], r, case["data"][p], gpu["coeffs"][i, b], host["coeffs"][i, b])
            a_err = max(8 * s_err, 2 * FLOOR + 2.0 ** -23 * float(host["error"][i, b]))
            a_curve = max(8 * s_curve,
                          FLOOR + 2.0 ** -23 * _term_norms(host["sigmas"], r, case["data"][p], host["coeffs"][i, b]))
            m_err, m_curve = max(m_err, d_err), max(m_curve, d_curve)
            w_err, w_curve = max(w_err, d_err / a_err), max(w_curve, d_curve / a_curve)
    print("desired %d: GPU vs host: error diff %.3e (%.3f of its allowance), curve diff %.3e (%.3f of its allowance)"
          % (dl, m_err, w_err, m_curve, w_curve))
    assert w_err <= 1.0
    assert w_curve <= 1.0
    # rgb rows are ToRGBSpectrum of the returned coefficients; rows outside every chosen window are zero
    used = np.zeros(len(host["sigmas"]), bool)
    for c in np.unique(gpu["centre"]):
        used[c - 3:c + 3] = True
    assert not gpu["coeffs"][:, :, ~used].any() and not gpu["rgb_coeffs"][:, :, ~used].any()


@pytest.mark.parametrize("dl", DESIRED)
def test_id_range_returns_the_same_rows(mpss, ctx, full, dl):
    part = ctx.profile_fit(mpss.profile_fit_spec(desired_length=dl, id_range=(3, 7), **sog_ref.GRID))
    assert part["coeffs"].shape[0] == 4
    assert part["sigmas"].tobytes() == full[dl]["sigmas"].tobytes()  # the sigma list is the whole grid's
    for k in ("coeffs", "error", "rgb_coeffs", "centre"):
        assert part[k].tobytes() == full[dl][k][3:7].tobytes(), k


def test_stage_times_and_empty_range(mpss, ctx):
    r = ctx.profile_fit(mpss.profile_fit_spec(desired_length=16, **sog_ref.GRID), timing=True)
    assert r["stage_ms"][0] > 0 and r["stage_ms"][1] > 0 and r["batches"] == 1
    one = ctx.profile_fit(mpss.profile_fit_spec(desired_length=16, max_profiles_per_batch=1, id_range=(2, 3),
                                                **sog_ref.GRID), timing=True)
    assert one["batches"] == 30  # one channel per batch
    e = ctx.profile_fit(mpss.profile_fit_spec(desired_length=16, id_range=(5, 5), **sog_ref.GRID))
    assert e["coeffs"].shape[0] == 0 and len(e["sigmas"]) == len(r["sigmas"])
