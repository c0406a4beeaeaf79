// profile_fit.cpp -- host side of Renderer "multipoleprofilefit": see profile_fit.h. Plain C++.
#include "profile_fit.h"

#include <cmath>
#include <limits>

#include "sog_math.h"

namespace mpss {

int fit_profile_samples_host(int desired_length) {
    unsigned len = 1;
    while (len < (unsigned)desired_length) len <<= 1;
    const unsigned ext = len - 1;
    std::vector<unsigned char> seen((size_t)ext * ext + 1, 0);
    int n = 0;
    for (unsigned i = 0; i <= ext; ++i)
        for (unsigned j = i; i * i + j * j <= ext * ext; ++j)
            if (!seen[i * i + j * j]) {
                seen[i * i + j * j] = 1;
                ++n;
            }
    return n;
}

void fit_params_from_id(uint32_t id, const float *const ranges[4], const uint32_t n[4], float out[4]) {
    for (int k = 3; k >= 0; --k) {  // NextParamFromId: f_ohg first
        out[k] = ranges[k][id % n[k]];
        id /= n[k];
    }
}

std::vector<float> fit_sigma_list(float mfp_min, float mfp_max) {
    std::vector<float> s;
    if (!(mfp_min > 0.f) || !std::isfinite(mfp_max)) return s;
    for (float sigma = mfp_min / 8.f; sigma <= mfp_max * 8.f; sigma *= 2.f) s.push_back(sigma);
    return s;
}

void sog_candidates(int n_sigmas, const float *sigmas, float mfp_min, float mfp_max, int &first, int &count) {
    first = 0;
    count = 0;
    for (int c = kSogNeg; c < n_sigmas - (kSogTerms - kSogNeg - 1); ++c) {
        const float sigma = sigmas[c];
        if (sigma < mfp_min / 2.f) continue;
        if (sigma > mfp_max * 2.f) break;
        if (!count) first = c;
        ++count;
    }
}

void sog_solve6(const double a[36], const double b[6], double x[6], bool quirk) { sog_solve6_impl(a, b, x, quirk); }

void sog_fit_window(uint32_t length, const float *dist_sq, const float *data, const float *sig, float coeff[6],
                    float *err, double *gram) {
    double X[36], Y[6], B[6];
    for (int i = 0; i < 36; ++i) X[i] = 0;
    for (int i = 0; i < 6; ++i) Y[i] = 0;
    for (uint32_t i = 0; i < length; ++i) {
        const double xi = sqrtf(dist_sq[i]);
        const double yi = data[i];
        double G[6];
        for (int j = 0; j < 6; ++j) G[j] = sog_gauss(xi, sig[j]);
        for (int j = 0; j < 6; ++j) {
            Y[j] += G[j] * yi;
            for (int k = 0; k < 6; ++k) X[j * 6 + k] += G[j] * G[k];
        }
    }
    sog_solve6_impl(X, Y, B, true);
    double error = 0, total = 0, prev = 0;
    for (uint32_t i = 0; i < length; ++i) {
        const double xi = sqrtf(dist_sq[i]);
        const double yi = data[i];
        double fitted = 0;
        for (int j = 0; j < 6; ++j) fitted += B[j] * sog_gauss(xi, sig[j]);
        error += xi * (fitted - yi) * (fitted - yi) * (xi - prev);
        total += xi * yi * yi * (xi - prev);
        prev = xi;
    }
    *err = (float)sqrt(error / total);
    for (int k = 0; k < 6; ++k) coeff[k] = sog_normalised(B[k], sig[k]);
    if (gram)
        for (int i = 0; i < 36; ++i) gram[i] = X[i];
}

int sog_select(int first, int count, const float *cand_error_row) {
    float min_err = std::numeric_limits<float>::infinity();
    int best = -1;  // (the reference would read a null cache entry when nothing was below infinity)
    for (int c = first; c < first + count; ++c)
        if (cand_error_row[c] < min_err) {
            min_err = cand_error_row[c];
            best = c;
        }
    return best;
}

int64_t sog_fit_host(uint32_t n, uint32_t length, const float *dist_sq, const float *data, int n_sigmas,
                     const float *sigmas, const float *mfp_min, const float *mfp_max, float *coeffs, float *error,
                     int32_t *centre, float *cand_error, float *cand_coeffs, double *cand_gram) {
    int64_t bad = -1;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> errs((size_t)n_sigmas), cf((size_t)n_sigmas * 6);
    for (uint32_t p = 0; p < n; ++p) {
        const float *d = dist_sq + (size_t)p * length, *y = data + (size_t)p * length;
        int first, count;
        sog_candidates(n_sigmas, sigmas, mfp_min[p], mfp_max[p], first, count);
        for (int c = 0; c < n_sigmas; ++c) errs[c] = nan;
        for (size_t k = 0; k < cf.size(); ++k) cf[k] = 0.f;
        for (int c = first; c < first + count; ++c)
            sog_fit_window(length, d, y, sigmas + c - kSogNeg, &cf[(size_t)c * 6], &errs[c],
                           cand_gram ? cand_gram + ((size_t)p * n_sigmas + c) * 36 : nullptr);
        const int best = sog_select(first, count, errs.data());
        for (int c = 0; c < n_sigmas; ++c) coeffs[(size_t)p * n_sigmas + c] = 0.f;
        centre[p] = best;
        error[p] = best >= 0 ? errs[best] : nan;
        if (best >= 0)
            for (int k = 0; k < 6; ++k) coeffs[(size_t)p * n_sigmas + best - kSogNeg + k] = cf[(size_t)best * 6 + k];
        else if (bad < 0)
            bad = p;
        if (cand_error)
            for (int c = 0; c < n_sigmas; ++c) cand_error[(size_t)p * n_sigmas + c] = errs[c];
        if (cand_coeffs)
            for (size_t k = 0; k < cf.size(); ++k) cand_coeffs[(size_t)p * n_sigmas * 6 + k] = cf[k];
    }
    return bad;
}

}  // namespace mpss
