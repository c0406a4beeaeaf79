"""The sum-of-Gaussians fit on the CPU: the library's host restatement (csrc/profile_fit.cpp, mpss_host_sog_fit,
mpss_host_profile_fit) against the float64 numpy restatement of GF_FitSumGaussians / DoGaussianFit in
tests/sog_ref.py, the sigma list, the id mapping and the text table of mpss/profilefit.py.

Bit identity: both sides run the same FP64 arithmetic in the same order (exp through the C library on both),
so every float output is compared bit for bit. The one exception is a NaN (a window whose elimination met a
zero pivot): NaNs compare as equal whatever their sign and payload, which the two languages' 0/0 do not fix.
"""
import io

import numpy as np
import pytest

import sog_ref


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)))) and \
        np.array_equal(np.signbit(a)[~np.isnan(a)], np.signbit(b)[~np.isnan(b)])


def test_exact_recovery_of_six_gaussians(mpss):
    """87 points uniform in d^2 (the sample count at desired_length 16); data = a known sum of the window's 6
    Gaussians: the host fit returns those coefficients and an error at float rounding."""
    sig = (0.05 * 2.0 ** np.arange(8)).astype(np.float32)
    d2 = (np.arange(87, dtype=np.float32) * np.float32(3.0 ** 2) / np.float32(86)).astype(np.float32)
    r = np.sqrt(d2).astype(np.float64)
    k_true = np.array([0.3, 0.25, 0.2, 0.12, 0.08, 0.05])  # normalised coefficients of sigmas[1..6]
    y = np.zeros(87)
    for s, k in zip(sig[1:7].astype(np.float64), k_true):
        y += k / (2 * np.pi * s * s) * np.exp(-r * r / (2 * s * s))
    # mfp bounds that admit the single centre 4 (window sigmas[1..6]): sigma_4 / 2 <= ... <= 2 sigma_4
    out = mpss.host_sog_fit(d2, y.astype(np.float32), sig, float(sig[4]) * 1.5, float(sig[4]) / 1.5, gram=True)
    assert out["centre"][0] == 4
    kappa = np.linalg.cond(out["cand_gram"][0, 4])
    # float data (2^-24 relative) through a system of condition kappa
    assert np.abs(out["coeffs"][0, 1:7] - k_true).max() <= max(1e-5, 4 * kappa * 2.0 ** -24) * k_true.max(), kappa
    assert out["coeffs"][0, 0] == 0 and out["coeffs"][0, 7] == 0
    assert out["error"][0] < 1e-5


@pytest.fixture(scope="module")
def oracle_profiles(mpss, oracle):
    """(d^2, R, sigmas, mfp_min, mfp_max) of a few bands of three layer sets at 87, 318 and 1162 samples, built
    by the oracle (o_mpc_profile + o_mpc_resample_uniform)."""
    fits = [mpss.profile_fit_spec(desired_length=16, **sog_ref.GRID),
            mpss.profile_fit_spec(desired_length=16, layer_thickness_nm=(0.1e6, 5e6), layer_ior=(1.3, 1.5), **sog_ref.GRID)]
    sig = mpss.host_profile_fit(fits[0])["sigmas"]
    out = []
    for dl, L in ((16, 87), (32, 318), (64, 1162)):
        for fit, ident, bands in ((fits[0], 0, (0, 9, 18)), (fits[0], 6, (5, 20)), (fits[1], 2, (7, 25))):
            mua, musp, th, eta = mpss.profilefit_layers(fit, ident)
            for b in bands:
                d, y = sog_ref.oracle_fit_profile(oracle, [(mua[l, b], musp[l, b], eta[l], th[l]) for l in range(2)], dl)
                assert len(d) == L
                mfp = np.float32(1) / (mua[:, b] + musp[:, b])
                out.append((d, y, sig, mfp.min(), mfp.max()))
    return out


def test_host_fit_matches_numpy_restatement_bit_for_bit(mpss, oracle_profiles):
    n_cand = 0
    for d, y, sig, lo, hi in oracle_profiles:
        lib = mpss.host_sog_fit(d, y, sig, lo, hi, gram=True)
        ref = sog_ref.fit_profile(d, y, sig, lo, hi)
        assert ref["cand"] == [c for c in range(len(sig)) if lib["cand_gram"][0, c].any()]
        for c in ref["cand"]:
            assert np.array_equal(lib["cand_gram"][0, c], ref["gram"][c]), c
            assert _same(lib["cand_coeffs"][0, c], ref["cand_coeffs"][c]), (c, lib["cand_coeffs"][0, c])
            assert _same(lib["cand_error"][0, c], ref["cand_error"][c]), c
            n_cand += 1
        assert lib["centre"][0] == ref["centre"]
        assert _same(lib["coeffs"][0], ref["coeffs"]) and _same(lib["error"][0], ref["error"])
    assert n_cand > 60


def test_pivot_quirk_is_visible_and_kept(mpss, oracle_profiles):
    """A window where searching the pivot in the partly eliminated matrix (a textbook solver) gives other float
    coefficients: the library gives the reference's."""
    seen = 0
    for d, y, sig, lo, hi in oracle_profiles:
        quirk = sog_ref.fit_profile(d, y, sig, lo, hi, quirk=True)
        plain = sog_ref.fit_profile(d, y, sig, lo, hi, quirk=False)
        lib = mpss.host_sog_fit(d, y, sig, lo, hi, gram=True)
        for c in quirk["cand"]:
            a, b = quirk["cand_coeffs"][c], plain["cand_coeffs"][c]
            if np.isfinite(a).all() and np.isfinite(b).all() and not np.array_equal(a, b):
                assert np.array_equal(lib["cand_coeffs"][0, c], a)
                # and the library's solver with the quirk switched off is the textbook one
                X = lib["cand_gram"][0, c]
                rhs = X @ np.ones(6)
                assert np.array_equal(mpss.host_sog_solve(X, rhs, quirk=False), sog_ref.linear_solve(X, rhs, quirk=False))
                assert np.array_equal(mpss.host_sog_solve(X, rhs, quirk=True), sog_ref.linear_solve(X, rhs, quirk=True))
                seen += 1
    assert seen > 0, "no window among the inputs shows the quirk"


def test_sigma_list_ids_and_range_clipping(mpss):
    fit = mpss.profile_fit_spec(desired_length=16, f_mel=[0.1, 0.01], f_eu=[0.5], f_blood=[0.05, 0.002], f_ohg=[0.9, 0.3])
    # ranges are sorted; f_mel outermost, f_ohg innermost
    want = [(m, 0.5, b, o) for m in (0.01, 0.1) for b in (0.002, 0.05) for o in (0.3, 0.9)]
    for i, w in enumerate(want):
        assert np.array_equal(mpss.profilefit_params(fit, i), np.array(w, np.float32))
    with pytest.raises(mpss.MpssError):
        mpss.profilefit_params(fit, 8)
    # sigma list: min / max of 10 / (mua + musp) [1 / cm -> mm] over the 61 wavelength entries of both layers of
    # the whole grid, then doubling from min / 8 while <= max * 8, in float. The 61-entry range contains the
    # 30 bands' (band values are averages of the entries).
    full = mpss.host_profile_fit(fit)
    sig = full["sigmas"]
    assert np.array_equal(sig[1:], (sig[:-1] * np.float32(2)).astype(np.float32))
    lo, hi = mpss.profilefit_mfp_bounds(fit, range(8))
    assert sig[0] * 8 <= lo.min() and sig[-1] <= hi.max() * 8 < sig[-1] * 2
    assert np.array_equal(sig, sog_ref.sigma_list(sig[0] * np.float32(8), hi.max())[:len(sig)])
    assert full["coeffs"].shape == (8, 30, len(sig)) and full["rgb_coeffs"].shape == (8, 3, len(sig))
    # idrange clipping (DoProfileFit :309-311)
    for rng, rows in (((3, 7), range(3, 7)), ((-2, 2), range(0, 2)), ((6, 100), range(6, 8)), ((0, -1), range(8)),
                      ((5, 5), range(0)), ((7, 3), range(0))):
        part = mpss.host_profile_fit(mpss.profile_fit_spec(desired_length=16, id_range=rng, **sog_ref.GRID))
        assert part["sigmas"].tobytes() == sig.tobytes()  # the sigma list is the whole grid's
        assert part["coeffs"].tobytes() == full["coeffs"][list(rows)].tobytes(), rng
        assert part["centre"].tobytes() == full["centre"][list(rows)].tobytes(), rng
    # the rgb rows are ToRGBSpectrum of each sigma's 30 coefficients
    import oracle_lib
    oracle_lib.build()
    for s in range(len(sig)):
        assert np.array_equal(full["rgb_coeffs"][2, :, s], oracle_lib.to_rgb(full["coeffs"][2, :, s]))


def test_sigma_list_runs_over_the_61_wavelength_entries(mpss):
    """The sigma list starts at (the least mfp of the grid) / 8, the least taken over the 61 entries of the
    wavelength-dependent values (400, 405, ... 700 nm; WLDValue::Min), not over the 30 bands. Computed here on
    its own from the skin model's formulas (skincoeffs.h): the least mfp of GRID is the epidermis at the most
    melanin, 10 / (mua_epi + musp_epi) [1 / cm -> mm] at 400 nm. float32 arithmetic in another association than
    the library's: 1e-5 relative. The 30 bands' least value (band 0 averages 400..410 nm) is 4 % larger."""
    fit = mpss.profile_fit_spec(desired_length=16, **sog_ref.GRID)
    sig = mpss.host_profile_fit(fit)["sigmas"]
    wl = (400 + 5 * np.arange(61)).astype(np.float64)
    base = 0.244 + 85.3 * np.exp(-(wl - 154) / 66.2)
    musp = 2e12 * wl ** -4.0 + 147.4 * wl ** -0.22
    least = np.inf
    for f_mel in sog_ref.GRID["f_mel"]:
        for f_eu in sog_ref.GRID["f_eu"]:
            mel = f_eu * 6.6e11 * wl ** -3.33 + (1 - f_eu) * 2.9e15 * wl ** -4.75
            least = min(least, (10 / (f_mel * mel + (1 - f_mel) * base + musp)).min())
    # (the dermis scatters half as much and, over this grid, absorbs less at every wavelength: its mfp is longer)
    assert abs(float(sig[0]) * 8 - least) <= 1e-5 * least, (float(sig[0]) * 8, least)
    lo, _ = mpss.profilefit_mfp_bounds(fit, range(8))  # the channels' own mfp: the 30 bands
    assert lo.min() > 1.02 * least  # the band values would have started the list visibly later
    # the list is that start doubled while <= 8 x the longest mfp; 61 entries or 30 bands, the longest is the
    # dermis at the red end, where the spectra are flat: the count follows from the two ends
    n = len(sig)
    assert sig[-1] == np.float32(sig[0] * np.float32(2.0 ** (n - 1)))


def test_fit_layers_are_the_skin_model_in_millimetres(mpss):
    """CreateGaussianFitTasks' units (profilefit.cpp:262-274): the band values of the 1 / cm coefficients over
    10, thickness (nm) over 1e6. mpss_host_skin_layers at nmperunit 1e7 multiplies the 61 entries by 1e7 / 1e7
    = 1 (exact) before it takes the band values, so its mua / musp are the 1 / cm band values bit for bit and
    the fit's layers must be exactly those over 10 in float."""
    fit = mpss.profile_fit_spec(desired_length=16, layer_thickness_nm=(0.1e6, 5e6), layer_ior=(1.3, 1.5), **sog_ref.GRID)
    for ident in (0, 3, 6):
        f_mel, f_eu, f_blood, f_ohg = mpss.profilefit_params(fit, ident)
        skin = mpss.default_skin(nmperunit=1e7, f_mel=float(f_mel), f_eu=float(f_eu), f_blood=float(f_blood),
                                 f_ohg=float(f_ohg), layer_thickness_nm=(0.1e6, 5e6), layer_ior=(1.3, 1.5))
        mua_cm, musp_cm, _, eta_ref = mpss.host_skin_layers(skin)
        mua, musp, th, eta = mpss.profilefit_layers(fit, ident)
        assert np.array_equal(mua, mua_cm / np.float32(10)) and np.array_equal(musp, musp_cm / np.float32(10))
        assert np.array_equal(th, np.array([0.1e6, 5e6], np.float32) / np.float32(1e6))
        assert np.array_equal(eta, eta_ref)
    # and not what nmperunit = 1e6 gives through the material path (x 0.1 before the band values): close, not equal
    skin = mpss.default_skin(nmperunit=1e6, f_mel=0.01, f_eu=0.5, f_blood=0.002, f_ohg=0.3)
    near = mpss.host_skin_layers(skin)[0]
    mine = mpss.profilefit_layers(mpss.profile_fit_spec(desired_length=16, **sog_ref.GRID), 0)[0]
    assert np.allclose(near, mine, rtol=1e-6) and not np.array_equal(near, mine)


def test_text_table_bytes(mpss):
    import mpss.profilefit as pf
    fit = mpss.profile_fit_spec(desired_length=16, id_range=(0, 2), **sog_ref.GRID)
    res = mpss.host_profile_fit(fit)
    buf = io.StringIO()
    pf.write_table(buf, sog_ref.GRID, res, id_min=0)
    lines = buf.getvalue().split("\n")
    assert lines[-1] == "" and len(lines) == 6 + 2 * 33 + 1
    assert lines[0] == "Param\tNum Samples\tSample Points"
    assert lines[1] == "f_mel\t2\t0.01\t0.1" and lines[2] == "f_eu\t1\t0.5"
    assert lines[3] == "f_blood\t2\t0.002\t0.05" and lines[4] == "f_ohg\t2\t0.3\t0.9"
    assert lines[5] == "ID\tf_mel\tf_eu\tf_blood\tf_ohg\tRGB\t" + "\t".join("%g" % s for s in res["sigmas"]) + "\tError"
    # first band row of id 0: wavelength 405 = the centre of band 0 (SampledSpectrum::WaveLength)
    row = lines[6].split("\t")
    assert row[:6] == ["0", "0.01", "0.5", "0.002", "0.3", "405"]
    assert row[6:-1] == ["%g" % v for v in res["coeffs"][0, 0]] and row[-1] == "%g" % res["error"][0, 0]
    assert lines[6 + 29].split("\t")[5] == "695"
    # the three RGB rows follow each id's 30 band rows and carry no error field
    for k, ch in enumerate("RGB"):
        row = lines[6 + 30 + k].split("\t")
        assert row[:6] == ["0", "0.01", "0.5", "0.002", "0.3", ch]
        assert row[6:] == ["%g" % v for v in res["rgb_coeffs"][0, k]]
    assert lines[6 + 33].split("\t")[:5] == ["1", "0.01", "0.5", "0.002", "0.9"]
    # without the header: a range that does not contain id 0
    fit2 = mpss.profile_fit_spec(desired_length=16, id_range=(1, 3), **sog_ref.GRID)
    res2 = mpss.host_profile_fit(fit2)
    buf2 = io.StringIO()
    pf.write_table(buf2, sog_ref.GRID, res2, id_min=1)
    lines2 = buf2.getvalue().split("\n")
    assert len(lines2) == 2 * 33 + 1 and lines2[0].startswith("1\t0.01\t0.5\t0.002\t0.9\t405\t")
    assert lines2[:33] == lines[6 + 33:6 + 66]


def test_error_statuses(mpss):
    d = np.linspace(0, 1, 87, dtype=np.float32)
    y = np.exp(-d).astype(np.float32)
    sig = (0.01 * 2.0 ** np.arange(10)).astype(np.float32)
    with pytest.raises(mpss.MpssError, match=r"error -2: .*no candidate"):
        mpss.host_sog_fit(d, y, sig, 1e3, 2e3)  # every sigma is below mfpMin / 2
    with pytest.raises(mpss.MpssError, match=r"error -1"):
        mpss.host_sog_fit(d, y, sig[:5], 0.1, 0.2)  # fewer than 6 sigmas
    with pytest.raises(mpss.MpssError, match=r"error -1"):
        mpss.host_profile_fit(mpss.profile_fit_spec(desired_length=4096, **sog_ref.GRID))
    with pytest.raises(mpss.MpssError, match=r"error -1"):
        mpss.host_profile_fit(mpss.profile_fit_spec(desired_length=16, f_mel=[], f_eu=[0.5], f_blood=[0.002], f_ohg=[0.3]))
