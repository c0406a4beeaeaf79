// sog_fit.h -- the sum-of-Gaussians fit on the GPU (sog_fit.hip): DoGaussianFit (profilefit.cpp:203-255)
// over n device-resident profiles.
#pragma once
#include "common.h"

namespace mpss {

struct SogFitWork {  // device workspace: keep it alive until the stream has run the work
    DevBuf<float> sigmas, cand_error, cand_coeffs;  // cand_*: [capacity][n_sigmas] and [capacity][n_sigmas][6]
    DevBuf<int2> cand;                               // [n]: first candidate centre, candidate count
    int n_sigmas = 0, max_count = 0;
    uint32_t n = 0, capacity = 0;
};

// Everything of the fit that allocates or copies from the host, for n profiles fitted `capacity` at a time:
// the candidate windows of all n (laid out on the host, profile_fit.cpp's sog_candidates), the sigma list, the
// per-candidate workspace. It uses blocking copies: call it BEFORE the work the fit is to follow is queued.
void sog_fit_prepare(uint32_t n, uint32_t capacity, int n_sigmas, const float *sigmas, const float *mfp_min,
                     const float *mfp_max, SogFitWork &w);
// The fit of profiles p0 .. p0 + count - 1 (count <= capacity): memsets and kernels on `stream` only -- no
// allocation, no host copy, nothing waits. dist_sq_dev / data_dev: [count][length] (d^2 and R as the profile
// stage leaves them); outputs on the device: coeffs [count][n_sigmas], error [count], centre [count] (-1: no
// candidate). The per-candidate results stay in w.cand_error [count][n_sigmas] (NaN: no candidate) and
// w.cand_coeffs [count][n_sigmas][6] until the next launch.
void sog_fit_launch(uint32_t p0, uint32_t count, uint32_t length, const float *dist_sq_dev, const float *data_dev,
                    float *coeffs_dev, float *error_dev, int32_t *centre_dev, SogFitWork &w, hipStream_t stream);
// The whole fit of n host-resident profiles, arguments and result as sog_fit_host's (profile_fit.h): upload,
// prepare, one launch, copy back, wait.
int64_t sog_fit_gpu(uint32_t n, uint32_t length, const float *dist_sq, const float *data, int n_sigmas,
                    const float *sigmas, const float *mfp_min, const float *mfp_max, float *coeffs, float *error,
                    int32_t *centre, float *cand_error, float *cand_coeffs, hipStream_t stream);

}  // namespace mpss
