// profile_fit.h -- the host side of Renderer "multipoleprofilefit" (src/renderers/profilefit.cpp:158-379,
// src/multipole/MultipoleProfileCalculator/gaussianfit.cpp:42-154): id mapping, the sigma list, the
// candidate windows, and the sum-of-Gaussians fit restated in FP64 in the reference's own order. Plain
// C++: no HIP runtime, no device (tests/sog_host links it alone, as tests/cg_host links common_grid.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace mpss {

constexpr int kSogTerms = 6;  // nTargetSigmas (profilefit.cpp:205)
constexpr int kSogNeg = 3;    // sigmaNegExtent: a window is sigmas[centre - 3 .. centre + 2]

// samples of a profile at desired_length: the distinct i^2 + j^2 <= ext^2, 0 <= i <= j, ext = the next power
// of two - 1 (MultipoleProfileCalculator.cpp:316-330): 87 at 16, 1162 at 64, 15978 at 256
int fit_profile_samples_host(int desired_length);
// ParamsFromId (profilefit.cpp:95-107): f_ohg innermost, f_mel outermost; n[4] / out[4] in the order
// f_mel, f_eu, f_blood, f_ohg
void fit_params_from_id(uint32_t id, const float *const ranges[4], const uint32_t n[4], float out[4]);
// the sigma list (DoProfileFit :303-307), in float: sigma = min / 8; sigma <= max * 8; sigma *= 2
std::vector<float> fit_sigma_list(float mfp_min, float mfp_max);
// DoGaussianFit's candidate centres (:222-225) for one profile: centres first .. first + count - 1
// (consecutive, because the sigmas ascend); count 0 when no sigma passes the mfp filter
void sog_candidates(int n_sigmas, const float *sigmas, float mfp_min, float mfp_max, int &first, int &count);

// GF_FitSumGaussians (gaussianfit.cpp:98-154) of one window of 6 sigmas: dist_sq / data are the resampled
// profile (d^2 and R); r = sqrtf(d^2) as DoGaussianFit takes it (:212-215). coeff = pNormalizedCoeffs,
// *err = overallError; gram (nullable) receives X row-major.
void sog_fit_window(uint32_t length, const float *dist_sq, const float *data, const float *sigmas6, float coeff[6],
                    float *err, double *gram);
// LinearSolve (gaussianfit.cpp:48-96) for 6 unknowns, pivot rows searched in the ORIGINAL matrix a (its
// quirk); quirk = false searches the partly eliminated matrix instead (a textbook partial pivot; the tests
// use it to show the difference)
void sog_solve6(const double a[36], const double b[6], double x[6], bool quirk = true);

// DoGaussianFit for n profiles of `length` samples. Outputs: coeffs [n][n_sigmas] (the chosen window's six,
// zero elsewhere), error [n], centre [n] (-1: no candidate); nullable: cand_error [n][n_sigmas] (NaN where
// the centre is no candidate), cand_coeffs [n][n_sigmas][6], cand_gram [n][n_sigmas][36].
// Returns the first profile without a candidate, or -1.
int64_t sog_fit_host(uint32_t n, uint32_t length, const float *dist_sq, const float *data, int n_sigmas,
                     const float *sigmas, const float *mfp_min, const float *mfp_max, float *coeffs, float *error,
                     int32_t *centre, float *cand_error, float *cand_coeffs, double *cand_gram);
// the selection alone (first candidate of least error, strict <, ascending centres) and the scatter
int sog_select(int first, int count, const float *cand_error_row);

}  // namespace mpss
