// sog_math.h -- the parts of the sum-of-Gaussians fit that the host restatement (profile_fit.cpp) and the
// fit kernel (sog_fit.hip) must compute alike: one copy, compiled for both. FP64, no contraction.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define MPSS_SOG_HD __host__ __device__ inline
#else
#define MPSS_SOG_HD inline
#endif

#pragma STDC FP_CONTRACT OFF

namespace mpss {

// GaussianFunc (gaussianfit.cpp:42-46): not normalised
MPSS_SOG_HD double sog_gauss(double r, double sigma) { return exp(-(r * r) / (2 * sigma * sigma)); }

// LinearSolve (gaussianfit.cpp:48-96), 6 unknowns. quirk: the pivot row is searched in the original matrix
// a, not in the partly eliminated aa (:58-63) -- the reference's behaviour, kept.
MPSS_SOG_HD void sog_solve6_impl(const double *a, const double *b, double *x, bool quirk) {
    double aa[36], bb[6];
    for (int i = 0; i < 36; ++i) aa[i] = a[i];
    for (int i = 0; i < 6; ++i) bb[i] = b[i];
    for (int row = 0; row < 5; ++row) {
        const double *s = quirk ? a : aa;
        int pivot = row;
        double max_abs = fabs(s[row * 6 + row]);
        for (int row2 = row + 1; row2 < 6; ++row2) {
            const double v = fabs(s[row2 * 6 + row]);
            if (v > max_abs) {
                max_abs = v;
                pivot = row2;
            }
        }
        if (max_abs > 0) {
            if (pivot != row) {
                for (int c = row; c < 6; ++c) {  // swapRow(row, pivotRow, row): columns from `row` on
                    const double t = aa[row * 6 + c];
                    aa[row * 6 + c] = aa[pivot * 6 + c];
                    aa[pivot * 6 + c] = t;
                }
                const double t = bb[row];
                bb[row] = bb[pivot];
                bb[pivot] = t;
            }
            const double div = aa[row * 6 + row];
            aa[row * 6 + row] = 1;
            for (int c = row + 1; c < 6; ++c) aa[row * 6 + c] /= div;
            bb[row] /= div;
            for (int row2 = row + 1; row2 < 6; ++row2) {
                for (int c2 = row + 1; c2 < 6; ++c2) aa[row2 * 6 + c2] -= aa[row2 * 6 + row] * aa[row * 6 + c2];
                bb[row2] -= aa[row2 * 6 + row] * bb[row];
            }
        }
    }
    for (int row = 5; row >= 0; --row) {
        double rem = bb[row];
        for (int c = 5; c != row; --c) rem -= aa[row * 6 + c] * x[c];
        x[row] = rem / aa[row * 6 + row];
    }
}

// pNormalizedCoeffs[k] = (float)(B[k] * 2 * PI * sigma * sigma), PI the MPC's float (numutil.h:45)
MPSS_SOG_HD float sog_normalised(double b, float sigma_f) {
    const double sigma = sigma_f;
    return (float)(b * 2 * (double)3.141592654f * sigma * sigma);
}

}  // namespace mpss
