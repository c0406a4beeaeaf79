// sog_fit.hip -- GF_FitSumGaussians (gaussianfit.cpp:98-154) over every candidate window of every profile.
//
//   sog_fit_kernel     one workgroup (256 threads, 4 waves) per (profile, candidate centre). Pass 1: each
//                      thread takes samples i = tid, tid + 256, ... and keeps the 21 distinct entries of the
//                      symmetric 6 x 6 Gram matrix X and the 6 of Y in FP64 registers; a wave sums them with
//                      shuffles (offsets 32 .. 1), the 4 wave sums meet in LDS and thread 0 adds them in wave
//                      order, solves X B = Y (LinearSolve with its pivot quirk, sog_math.h) and leaves B in
//                      LDS. Pass 2: the error term's two sums the same way. The summation order is fixed by
//                      (length, thread count) alone, so a profile's result does not depend on what else is in
//                      the launch; it differs from the reference's sequential order by FP64 rounding.
//   sog_select_kernel  one thread per profile: first candidate of least overallError (strict <, ascending
//                      centres), its six coefficients scattered into the n_sigmas-wide row.
#include <vector>

#include "profile_fit.h"
#include "sog_fit.h"
#include "sog_math.h"

namespace mpss {

namespace {

constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kGramSums = 27;  // 21 entries X[j][k], j <= k, then Y[0..5]

template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*part)[kGramSums], double *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double x = v[k];
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) part[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < NV; ++k) {
            double s = part[0][k];
            for (int w = 1; w < kFitWaves; ++w) s += part[w][k];
            out[k] = s;
        }
    __syncthreads();
}

__global__ __launch_bounds__(kFitThreads) void sog_fit_kernel(const float *__restrict__ dist_sq,
                                                              const float *__restrict__ data, uint32_t length,
                                                              int n_sigmas, const float *__restrict__ sigmas,
                                                              const int2 *__restrict__ cand, float *cand_error,
                                                              float *cand_coeffs) {
    __shared__ double part[kFitWaves][kGramSums];
    __shared__ double sums[kGramSums];
    __shared__ double sB[6];
    const uint32_t p = blockIdx.x;
    const int2 fc = cand[p];
    if ((int)blockIdx.y >= fc.y) return;  // (uniform over the workgroup)
    const int c = fc.x + (int)blockIdx.y;
    const float *d = dist_sq + (size_t)p * length, *y = data + (size_t)p * length;
    float sig[6];
    for (int j = 0; j < 6; ++j) sig[j] = sigmas[c - kSogNeg + j];

    double acc[kGramSums];
#pragma unroll
    for (int k = 0; k < kGramSums; ++k) acc[k] = 0.;
    for (uint32_t i = threadIdx.x; i < length; i += kFitThreads) {
        const double xi = sqrtf(d[i]);
        const double yi = y[i];
        double G[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) G[j] = sog_gauss(xi, sig[j]);
        int at = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int k = j; k < 6; ++k) acc[at++] += G[j] * G[k];
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[21 + j] += G[j] * yi;
    }
    block_sum<kGramSums>(acc, part, sums);
    if (threadIdx.x == 0) {
        double X[36], B[6];
        int at = 0;
        for (int j = 0; j < 6; ++j)
            for (int k = j; k < 6; ++k) {
                X[j * 6 + k] = sums[at];
                X[k * 6 + j] = sums[at];
                ++at;
            }
        sog_solve6_impl(X, sums + 21, B, true);
        for (int j = 0; j < 6; ++j) sB[j] = B[j];
    }
    __syncthreads();
    double B[6];
    for (int j = 0; j < 6; ++j) B[j] = sB[j];
    double et[2] = {0., 0.};
    for (uint32_t i = threadIdx.x; i < length; i += kFitThreads) {
        const double xi = sqrtf(d[i]);
        const double prev = i ? (double)sqrtf(d[i - 1]) : 0.;
        const double yi = y[i];
        double fitted = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) fitted += B[j] * sog_gauss(xi, sig[j]);
        et[0] += xi * (fitted - yi) * (fitted - yi) * (xi - prev);
        et[1] += xi * yi * yi * (xi - prev);
    }
    __syncthreads();  // (thread 0 has read sums[21..26]; block_sum writes sums[0..1])
    block_sum<2>(et, part, sums);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)p * n_sigmas + c;
        cand_error[o] = (float)sqrt(sums[0] / sums[1]);
        for (int k = 0; k < 6; ++k) cand_coeffs[o * 6 + k] = sog_normalised(B[k], sig[k]);
    }
}

__global__ void sog_select_kernel(uint32_t n, int n_sigmas, const int2 *__restrict__ cand,
                                  const float *__restrict__ cand_error, const float *__restrict__ cand_coeffs,
                                  float *coeffs, float *error, int32_t *centre) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int2 fc = cand[p];
    const float *e = cand_error + (size_t)p * n_sigmas;
    float min_err = INFINITY;
    int best = -1;
    for (int c = fc.x; c < fc.x + fc.y; ++c)
        if (e[c] < min_err) {
            min_err = e[c];
            best = c;
        }
    float *row = coeffs + (size_t)p * n_sigmas;
    for (int c = 0; c < n_sigmas; ++c) row[c] = 0.f;
    centre[p] = best;
    error[p] = best >= 0 ? e[best] : NAN;
    if (best >= 0)
        for (int k = 0; k < 6; ++k) row[best - kSogNeg + k] = cand_coeffs[((size_t)p * n_sigmas + best) * 6 + k];
}

}  // namespace

void sog_fit_prepare(uint32_t n, uint32_t capacity, int n_sigmas, const float *sigmas, const float *mfp_min,
                     const float *mfp_max, SogFitWork &w) {
    if (n_sigmas < kSogTerms || n_sigmas > 4096) throw Error(-1, "sog_fit: needs 6 .. 4096 sigmas");
    if (n < 1 || capacity < 1) throw Error(-1, "sog_fit: no profiles");
    std::vector<int2> cand(n);
    w.max_count = 0;
    for (uint32_t p = 0; p < n; ++p) {
        int first, count;
        sog_candidates(n_sigmas, sigmas, mfp_min[p], mfp_max[p], first, count);
        cand[p] = make_int2(first, count);  // first >= 3 and first + count <= n_sigmas - 2: windows stay inside
        w.max_count = count > w.max_count ? count : w.max_count;
    }
    w.n = n;
    w.capacity = capacity < n ? capacity : n;
    w.n_sigmas = n_sigmas;
    w.sigmas.upload(sigmas, (size_t)n_sigmas);
    w.cand.upload(cand.data(), cand.size());
    w.cand_error.alloc((size_t)w.capacity * n_sigmas);
    w.cand_coeffs.alloc((size_t)w.capacity * n_sigmas * 6);
}

void sog_fit_launch(uint32_t p0, uint32_t count, uint32_t length, const float *dist_sq_dev, const float *data_dev,
                    float *coeffs_dev, float *error_dev, int32_t *centre_dev, SogFitWork &w, hipStream_t stream) {
    if (count == 0) return;
    if (count > w.capacity || (uint64_t)p0 + count > w.n) throw Error(-1, "sog_fit_launch: range outside the prepared work");
    if (length < 1) throw Error(-1, "sog_fit_launch: empty profiles");
    const int ns = w.n_sigmas;
    MPSS_HIP(hipMemsetAsync(w.cand_error.ptr, 0xff, sizeof(float) * (size_t)count * ns, stream));  // NaN
    MPSS_HIP(hipMemsetAsync(w.cand_coeffs.ptr, 0, sizeof(float) * (size_t)count * ns * 6, stream));
    if (w.max_count > 0)
        hipLaunchKernelGGL(sog_fit_kernel, dim3(count, (unsigned)w.max_count), dim3(kFitThreads), 0, stream, dist_sq_dev,
                           data_dev, length, ns, w.sigmas.ptr, w.cand.ptr + p0, w.cand_error.ptr, w.cand_coeffs.ptr);
    hipLaunchKernelGGL(sog_select_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, count, ns, w.cand.ptr + p0,
                       w.cand_error.ptr, w.cand_coeffs.ptr, coeffs_dev, error_dev, centre_dev);
    MPSS_HIP(hipGetLastError());
}

int64_t sog_fit_gpu(uint32_t n, uint32_t length, const float *dist_sq, const float *data, int n_sigmas,
                    const float *sigmas, const float *mfp_min, const float *mfp_max, float *coeffs, float *error,
                    int32_t *centre, float *cand_error, float *cand_coeffs, hipStream_t st) {
    const size_t cells = (size_t)n * length, ns = (size_t)n_sigmas;
    DevBuf<float> d_d, d_y, d_coeffs, d_err;
    DevBuf<int32_t> d_centre;
    d_d.upload(dist_sq, cells);
    d_y.upload(data, cells);
    d_coeffs.alloc(n * ns);
    d_err.alloc(n);
    d_centre.alloc(n);
    SogFitWork w;
    sog_fit_prepare(n, n, n_sigmas, sigmas, mfp_min, mfp_max, w);
    sog_fit_launch(0, n, length, d_d.ptr, d_y.ptr, d_coeffs.ptr, d_err.ptr, d_centre.ptr, w, st);
    MPSS_HIP(hipMemcpyAsync(coeffs, d_coeffs.ptr, sizeof(float) * n * ns, hipMemcpyDeviceToHost, st));
    MPSS_HIP(hipMemcpyAsync(error, d_err.ptr, sizeof(float) * n, hipMemcpyDeviceToHost, st));
    MPSS_HIP(hipMemcpyAsync(centre, d_centre.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (cand_error)
        MPSS_HIP(hipMemcpyAsync(cand_error, w.cand_error.ptr, sizeof(float) * n * ns, hipMemcpyDeviceToHost, st));
    if (cand_coeffs)
        MPSS_HIP(hipMemcpyAsync(cand_coeffs, w.cand_coeffs.ptr, sizeof(float) * n * ns * 6, hipMemcpyDeviceToHost, st));
    MPSS_HIP(hipStreamSynchronize(st));
    for (uint32_t p = 0; p < n; ++p)
        if (centre[p] < 0) return p;
    return -1;
}

}  // namespace mpss
