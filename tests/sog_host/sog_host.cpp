// sog_host.cpp -- stand-alone driver of csrc/profile_fit.cpp (plain C++: no libmpss, no HIP runtime, no GPU)
// for the sanitizer build of tests/test_sog_fit_sanitized.py: the host sum-of-Gaussians fit, the candidate
// filter, the sigma list and the id mapping on fixed inputs. Prints one line per case; exit 0 when all is well.
#include <cmath>
#include <cstdio>
#include <vector>

#include "profile_fit.h"

using namespace mpss;

int main() {
    int fails = 0;
    const std::vector<float> sig = fit_sigma_list(0.04f, 1.1f);
    std::printf("sigmas %zu first %g last %g\n", sig.size(), sig.front(), sig.back());
    if (sig.size() != 11) ++fails;  // 0.005 * 2^k <= 8.8
    for (int length : {1, 2, 87, 1162}) {
        const uint32_t n = 3;
        std::vector<float> d((size_t)n * length), y((size_t)n * length), lo(n), hi(n);
        for (uint32_t p = 0; p < n; ++p) {
            for (int i = 0; i < length; ++i) {
                const float d2 = length > 1 ? 9.f * (float)i / (float)(length - 1) : 0.f;
                d[(size_t)p * length + i] = d2;
                y[(size_t)p * length + i] = 0.3f * std::exp(-d2 / (0.1f + 0.2f * p)) + 0.01f * std::exp(-d2 / 2.f);
            }
            lo[p] = 0.05f * (float)(1 + p);
            hi[p] = 0.4f * (float)(1 + p);
        }
        hi[2] = 1e-4f;  // no sigma passes: this profile has no candidate
        const int ns = (int)sig.size();
        std::vector<float> coeffs((size_t)n * ns), err(n), ce((size_t)n * ns), cc((size_t)n * ns * 6);
        std::vector<int32_t> centre(n);
        std::vector<double> gram((size_t)n * ns * 36, 0.);
        const int64_t bad = sog_fit_host(n, (uint32_t)length, d.data(), y.data(), ns, sig.data(), lo.data(), hi.data(),
                                         coeffs.data(), err.data(), centre.data(), ce.data(), cc.data(), gram.data());
        std::printf("length %d centres %d %d %d errors %g %g bad %lld\n", length, centre[0], centre[1], centre[2],
                    err[0], err[1], (long long)bad);
        // one or two samples: total = 0, every overallError is NaN and nothing is chosen (no crash)
        if (bad != (length < 87 ? 0 : 2) || centre[2] != -1) ++fails;
        if (length >= 87 && (centre[0] < 3 || centre[0] > ns - 3 || !(err[0] < 0.1f))) ++fails;
    }
    const float r0[] = {0.1f, 0.2f}, r1[] = {0.5f}, r2[] = {1.f, 2.f, 3.f}, r3[] = {7.f, 8.f};
    const float *const ranges[4] = {r0, r1, r2, r3};
    const uint32_t cnt[4] = {2, 1, 3, 2};
    float out[4];
    fit_params_from_id(11, ranges, cnt, out);
    std::printf("id 11 -> %g %g %g %g\n", out[0], out[1], out[2], out[3]);
    if (out[0] != 0.2f || out[2] != 3.f || out[3] != 8.f) ++fails;
    const double a[36] = {4, 1, 0, 0, 0, 0, 1, 4, 1, 0, 0, 0, 0, 1, 4, 1, 0, 0, 0, 0, 1, 4, 1, 0, 0, 0, 0, 1, 4, 1, 0, 0, 0, 0, 1, 4};
    const double b[6] = {5, 6, 6, 6, 6, 5};
    double x[6];
    sog_solve6(a, b, x, true);
    for (int i = 0; i < 6; ++i)
        if (std::fabs(x[i] - 1.) > 1e-12) ++fails;
    std::printf("fit profile samples %d %d\n", fit_profile_samples_host(16), fit_profile_samples_host(64));
    if (fit_profile_samples_host(16) != 87) ++fails;
    std::printf(fails ? "FAILED %d\n" : "all ok %d\n", fails);
    return fails ? 1 : 0;
}
