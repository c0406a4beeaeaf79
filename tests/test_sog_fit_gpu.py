"""The sum-of-Gaussians fit kernel (csrc/sog_fit.hip, mpss_sog_fit) against the library's host restatement
(mpss_host_sog_fit, itself checked against the numpy restatement in tests/test_sog_fit.py) on identical inputs:
the 240 profiles of sog_ref.GRID at 87 and 1162 samples, and one profile of 15978 samples (the sample count at
desiredProfileLength 256, built by the oracle).

The kernel sums the Gram matrix in another order (per-thread strided partial sums, wave shuffles, four wave sums
in LDS), so its coefficients may differ from the host's by the conditioning of the window:
    |coeff_gpu - coeff_host| <= max(4 * 2^-24, K * kappa * 2^-53) * max|coeff_host|   (per candidate)
with kappa = cond_2(X) of the candidate's Gram matrix (numpy). K is measured, not chosen: the numpy restatement
run with its Gram sums taken forwards and backwards (both reference arithmetic, neither the code under test);
K = 8 x the largest ratio of the difference of the two float64 normalised solutions to kappa * 2^-53 over the
candidates with kappa <= 1e8 of every fifth profile. Measured on the CPU: largest ratio 2.76 (87 samples), 2.06
(1162 samples), so K = 22.1 and 16.5. Candidates with kappa > 1e8 (a window reaching past the grid: kappa up to
1e19; most windows at 87 samples) are compared only through the final selection. The 15978-sample profile has
its own measurement (ratio 2.97 on the CPU, K = 23.8; printed by the test).

Each well-conditioned candidate's overallError is compared too. With a = fit_gpu - y and b = fit_host - y in
the error term's weighted norm, | ||a|| - ||b|| | <= ||a - b|| holds exactly, so the two errors may differ by
the distance of the two fitted curves (evaluated in float64 from the returned coefficients), plus what the
returned floats hide: one float rounding of each error (2^-24 of it each) and of each coefficient (2^-24 of the
summed term norms, each side).
"""
import numpy as np
import pytest

import sog_ref

pytestmark = pytest.mark.gpu

LENGTHS = {87: 16, 1162: 64}


@pytest.fixture(scope="module")
def ctx(mpss):
    c = mpss.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(mpss, ctx):
    out = {}
    for L, dl in LENGTHS.items():
        case = sog_ref.grid_case(mpss, dl)
        assert case["dist_sq"].shape == (240, L)
        gpu = ctx.sog_fit(case["dist_sq"], case["data"], case["host"]["sigmas"], case["mfp_min"], case["mfp_max"])
        out[L] = (case, gpu)
    return out


def _measure_k(case, profiles=range(0, 240, 5)):
    sig = case["host"]["sigmas"]
    worst = 0.0
    for p in profiles:
        a = (case["dist_sq"][p], case["data"][p], sig, case["mfp_min"][p], case["mfp_max"][p])
        fwd, bwd = sog_ref.fit_profile(*a), sog_ref.fit_profile(*a, reverse=True)
        for c in fwd["cand"]:
            kappa = np.linalg.cond(fwd["gram"][c])
            if kappa > 1e8:
                continue
            s2 = sig[c - 3:c + 3].astype(np.float64) ** 2
            x, y = fwd["B"][c] * s2, bwd["B"][c] * s2
            worst = max(worst, np.abs(x - y).max() / np.abs(x).max() / (kappa * 2.0 ** -53))
    return worst


def _error_allowance(sig, d2, y, h_row, g_row, h_err, g_err):
    """what two candidates' overallError may differ by (module docstring); rows: n_sigmas-wide coefficients"""
    r = np.sqrt(np.asarray(d2, np.float32)).astype(np.float64)
    return sog_ref.curve_distance(sig, r, y, g_row, h_row) + 2.0 ** -24 * (
        float(h_err) + float(g_err) + sog_ref.term_norms(sig, h_row, r, y) + sog_ref.term_norms(sig, g_row, r, y))


def _rows(sig, c, coeffs6):
    row = np.zeros(len(sig), np.float64)
    row[c - 3:c + 3] = coeffs6
    return row


@pytest.mark.parametrize("L", sorted(LENGTHS))
def test_candidates_within_conditioning_bound(runs, L):
    case, gpu = runs[L]
    host = case["sog"]
    ratio = _measure_k(case)
    K = 8 * ratio
    print("length %d: forward/backward ratio %.3f, K = %.2f" % (L, ratio, K))
    assert ratio > 0
    # a centre that is no candidate (the host left its Gram matrix untouched) has no result on the GPU either
    none = ~host["cand_gram"].any(axis=(2, 3))
    assert np.isnan(gpu["cand_error"][none]).all() and not gpu["cand_coeffs"][none].any()
    checked = skipped = 0
    worst = worst_e = 0.0
    for p in range(240):
        for c in range(host["cand_gram"].shape[1]):
            X = host["cand_gram"][p, c]
            if not X.any():
                continue
            kappa = np.linalg.cond(X) if np.isfinite(X).all() else np.inf
            if not kappa <= 1e8:
                skipped += 1
                continue
            h = host["cand_coeffs"][p, c].astype(np.float64)
            g = gpu["cand_coeffs"][p, c].astype(np.float64)
            tol = max(4 * 2.0 ** -24, K * kappa * 2.0 ** -53)
            rel = np.abs(g - h).max() / np.abs(h).max()
            worst = max(worst, rel / tol)
            assert rel <= tol, (p, c, kappa, rel, tol)
            he, ge = host["cand_error"][p, c], gpu["cand_error"][p, c]
            sig = case["host"]["sigmas"]
            allow = _error_allowance(sig, case["dist_sq"][p], case["data"][p], _rows(sig, c, h), _rows(sig, c, g), he, ge)
            worst_e = max(worst_e, abs(float(ge) - float(he)) / allow)
            assert abs(float(ge) - float(he)) <= allow, (p, c, he, ge, allow)
            checked += 1
    print("length %d: %d candidates checked, %d ill-conditioned left to the selection, worst coefficient diff / "
          "allowance %.3f, worst error diff / allowance %.3f" % (L, checked, skipped, worst, worst_e))
    assert checked > 0 and skipped > 0  # both kinds occur


@pytest.mark.parametrize("L", sorted(LENGTHS))
def test_chosen_centre_matches_host(runs, L):
    case, gpu = runs[L]
    host = case["sog"]
    amb = sog_ref.ambiguous(host["cand_error"])
    assert amb.mean() <= 0.02, amb.sum()
    assert np.array_equal(gpu["centre"][~amb], host["centre"][~amb])
    # where the centre agrees, the scattered row is the chosen candidate's and zero elsewhere
    for p in np.nonzero(~amb)[0]:
        c = gpu["centre"][p]
        row = np.zeros_like(gpu["coeffs"][p])
        row[c - 3:c + 3] = gpu["cand_coeffs"][p, c]
        assert np.array_equal(gpu["coeffs"][p], row, equal_nan=True)
        assert gpu["error"][p] == gpu["cand_error"][p, c]


def test_long_profile(mpss, ctx, oracle):
    """15978 samples: more than one pass of the workgroup over the samples per thread, the length of a
    desiredProfileLength-256 run."""
    fit = mpss.profile_fit_spec(desired_length=256, **sog_ref.GRID)
    mua, musp, th, eta = mpss.profilefit_layers(fit, 5)
    b = 12
    layers = [(mua[l, b], musp[l, b], eta[l], th[l]) for l in range(2)]
    d, y = sog_ref.oracle_fit_profile(oracle, layers, 256)
    assert len(d) == 15978
    sig = mpss.host_profile_fit(mpss.profile_fit_spec(desired_length=16, **sog_ref.GRID))["sigmas"]
    mfp = 1.0 / (mua[:, b] + musp[:, b])
    host = mpss.host_sog_fit(d, y, sig, mfp.min(), mfp.max(), gram=True)
    gpu = ctx.sog_fit(d, y, sig, mfp.min(), mfp.max())
    case = dict(dist_sq=d[None], data=y[None], mfp_min=[mfp.min()], mfp_max=[mfp.max()], host=dict(sigmas=sig))
    ratio = _measure_k(case, profiles=[0])
    K = 8 * ratio
    print("length 15978: forward/backward ratio %.3f, K = %.2f" % (ratio, K))
    assert ratio > 0
    n = 0
    for c in range(len(sig)):
        X = host["cand_gram"][0, c]
        if not X.any():
            continue
        kappa = np.linalg.cond(X)
        if kappa > 1e8:
            continue
        h = host["cand_coeffs"][0, c].astype(np.float64)
        g = gpu["cand_coeffs"][0, c].astype(np.float64)
        assert np.abs(g - h).max() / np.abs(h).max() <= max(4 * 2.0 ** -24, K * kappa * 2.0 ** -53), (c, kappa)
        he, ge = host["cand_error"][0, c], gpu["cand_error"][0, c]
        assert abs(float(ge) - float(he)) <= _error_allowance(sig, d, y, _rows(sig, c, h), _rows(sig, c, g), he, ge), c
        n += 1
    assert n > 0
    assert not sog_ref.ambiguous(host["cand_error"])[0]  # this profile's choice is no near-tie (checked on the CPU)
    assert gpu["centre"][0] == host["centre"][0]


def test_no_candidate_is_an_error_not_a_crash(mpss, ctx):
    d = np.linspace(0, 1, 87, dtype=np.float32)[None]
    y = np.exp(-d).astype(np.float32)
    sig = (0.01 * 2.0 ** np.arange(10)).astype(np.float32)
    with pytest.raises(mpss.MpssError, match="-2.*no candidate"):
        ctx.sog_fit(d, y, sig, 1e3, 2e3)
