// profile_fit_driver.cpp -- see profile_fit_driver.h. The plan needs material.cpp's skin_fit_*, which is why
// this is not part of profile_fit.cpp (that file links alone).
#include "profile_fit_driver.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>

#include "context.h"
#include "profile_fit.h"
#include "sog_fit.h"
#include "spectral.h"

namespace mpss {

namespace {

void require(bool ok, const char *msg) {
    if (!ok) throw Error(MPSS_ERR_INVALID, msg);
}

// DoProfileFit's setup (profilefit.cpp:284-312): sorted ranges, the sigma list over the whole grid, the
// clipped id range
struct FitPlan {
    std::vector<float> range[4];
    uint32_t n[4];
    uint32_t total = 0, id0 = 0, id1 = 0;
    std::vector<float> sigmas;
    // fit_layers: the layers of ids [id0, id1) in millimetres and every channel's own mfp bounds
    std::vector<LayerParams> lp;
    std::vector<float> mfp_min, mfp_max;
    void params(uint32_t id, float out[4]) const {
        const float *const r[4] = {range[0].data(), range[1].data(), range[2].data(), range[3].data()};
        fit_params_from_id(id, r, n, out);
    }
};

FitPlan make_fit_plan(const mpss_profilefit &f, bool with_sigmas = true) {
    FitPlan pl;
    const float *src[4] = {f.f_mel, f.f_eu, f.f_blood, f.f_ohg};
    const uint32_t cnt[4] = {f.n_f_mel, f.n_f_eu, f.n_f_blood, f.n_f_ohg};
    uint64_t total = 1;
    for (int k = 0; k < 4; ++k) {
        require(src[k] && cnt[k] >= 1, "profile fit: each of f_mel, f_eu, f_blood, f_ohg needs at least one value");
        pl.range[k].assign(src[k], src[k] + cnt[k]);
        std::sort(pl.range[k].begin(), pl.range[k].end());  // FindParamRange
        pl.n[k] = cnt[k];
        total *= cnt[k];
        require(total <= (1u << 20), "profile fit: more than 2^20 combinations");
    }
    require(f.desired_length >= 2 && f.desired_length <= 1024, "profile fit: desired_length outside 2..1024");
    for (int l = 0; l < 2; ++l)
        require(f.layer_thickness_nm[l] > 0.f && f.layer_ior[l] > 0.f, "profile fit: layers need thickness and ior > 0");
    pl.total = (uint32_t)total;
    float mfp_min = INFINITY, mfp_max = 0.f;
    for (uint32_t id = 0; with_sigmas && id < pl.total; ++id) {
        float v[4];
        pl.params(id, v);
        skin_fit_mfp_range(v[0], v[1], v[2], v[3], mfp_min, mfp_max);
    }
    if (with_sigmas) pl.sigmas = fit_sigma_list(mfp_min, mfp_max);
    pl.id0 = (uint32_t)std::max(0, f.id_min);
    pl.id1 = f.id_max < 0 ? pl.total : (uint32_t)std::min<int64_t>(pl.total, f.id_max);
    if (pl.id1 < pl.id0) pl.id1 = pl.id0;
    return pl;
}

// GaussianFitTask::Run :165-173
void fit_layers(const mpss_profilefit &f, FitPlan &pl) {
    const uint32_t n = pl.id1 - pl.id0;
    pl.lp.resize(n);
    pl.mfp_min.resize((size_t)n * NB);
    pl.mfp_max.resize((size_t)n * NB);
    for (uint32_t i = 0; i < n; ++i) {
        float v[4];
        pl.params(pl.id0 + i, v);
        skin_fit_layer_params(v[0], v[1], v[2], v[3], f.layer_thickness_nm, f.layer_ior, pl.lp[i]);
        for (int sc = 0; sc < NB; ++sc) {
            float lo = INFINITY, hi = 0.f;
            for (int l = 0; l < 2; ++l) {
                const float mfp = 1.f / (pl.lp[i].mua[l][sc] + pl.lp[i].musp[l][sc]);
                lo = std::min(lo, mfp);
                hi = std::max(hi, mfp);
            }
            pl.mfp_min[(size_t)i * NB + sc] = lo;
            pl.mfp_max[(size_t)i * NB + sc] = hi;
        }
    }
}

void fit_rgb_rows(uint32_t n_ids, uint32_t ns, const float *coeffs, float *rgb) {
    for (uint32_t i = 0; i < n_ids; ++i)
        for (uint32_t s = 0; s < ns; ++s) {
            float spec[NB], out[3];
            for (int sc = 0; sc < NB; ++sc) spec[sc] = coeffs[((size_t)i * NB + sc) * ns + s];
            spectrum_to_rgb(spec, out);
            for (int k = 0; k < 3; ++k) rgb[((size_t)i * 3 + k) * ns + s] = out[k];
        }
}

void fit_no_candidate(const FitPlan &pl, int64_t profile) {
    throw Error(MPSS_ERR_INTERNAL, "profile fit: id " + std::to_string(pl.id0 + profile / NB) + " band " +
                                       std::to_string(profile % NB) +
                                       " has no candidate window (no sigma within [mfpMin / 2, mfpMax * 2] "
                                       "with a full window around it)");
}

// what both fits start with: the plan's outputs and, unless nothing is to be fitted (false), the layers
bool fit_begin(const mpss_profilefit &f, FitPlan &pl, const char *who, uint32_t *n_sigmas, uint32_t *n_ids,
               float *sigmas, const float *coeffs) {
    *n_sigmas = (uint32_t)pl.sigmas.size();
    *n_ids = pl.id1 - pl.id0;
    if (sigmas) memcpy(sigmas, pl.sigmas.data(), sizeof(float) * pl.sigmas.size());
    if (!coeffs || *n_ids == 0) return false;
    fit_layers(f, pl);
    if (*n_sigmas < 6)
        throw Error(MPSS_ERR_INVALID, std::string(who) + ": the grid's mfp range gives fewer than 6 sigmas");
    return true;
}

// ... and end with
void fit_end(const FitPlan &pl, const std::vector<float> &err, const std::vector<int32_t> &cen, int64_t bad,
             const float *coeffs, float *error, int32_t *centre, float *rgb) {
    if (error) memcpy(error, err.data(), sizeof(float) * err.size());
    if (centre) memcpy(centre, cen.data(), sizeof(int32_t) * cen.size());
    if (bad >= 0) fit_no_candidate(pl, bad);
    if (rgb) fit_rgb_rows(pl.id1 - pl.id0, (uint32_t)pl.sigmas.size(), coeffs, rgb);
}

}  // namespace

void profile_fit_id(const char *who, const mpss_profilefit &f, uint32_t id, float v[4], LayerParams *lp) {
    const FitPlan pl = make_fit_plan(f, false);
    if (id >= pl.total) throw Error(MPSS_ERR_INVALID, std::string(who) + ": id out of range");
    pl.params(id, v);
    if (lp) skin_fit_layer_params(v[0], v[1], v[2], v[3], f.layer_thickness_nm, f.layer_ior, *lp);
}

void profile_fit_gpu(Context &ctx, const mpss_profilefit &f, uint32_t *n_sigmas, uint32_t *n_ids, float *sigmas,
                     float *coeffs, float *error, float *rgb, int32_t *centre, double *stage_ms, hipStream_t st) {
    FitPlan pl = make_fit_plan(f);
    if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = 0.;
    if (!fit_begin(f, pl, "mpss_profile_fit", n_sigmas, n_ids, sigmas, coeffs)) return;
    const uint32_t ns = *n_sigmas, P = *n_ids * NB;
    // a band without a candidate is known before anything is launched
    for (uint32_t p = 0; p < P; ++p) {
        int first, count;
        sog_candidates((int)ns, pl.sigmas.data(), pl.mfp_min[p], pl.mfp_max[p], first, count);
        if (!count) fit_no_candidate(pl, p);
    }
    auto lock = ctx.lock_device();
    // Every allocation and host copy of both stages happens here, before anything is queued: from the
    // first batch's memset to the copy back, the host only queues work on `st`. The workspaces live until
    // the wait below.
    GridWork pw;
    SogFitWork fw;
    const uint32_t batch = (uint32_t)fit_profiles_prepare(pl.lp.data(), (int)P, f.desired_length,
                                                          f.max_profiles_per_batch, pw);
    sog_fit_prepare(P, batch, (int)ns, pl.sigmas.data(), pl.mfp_min.data(), pl.mfp_max.data(), fw);
    const uint32_t nbatch = (P + batch - 1) / batch;
    const int nent = pw.plan.nent;
    DevBuf<float> d_d, d_y, d_coeffs, d_err;  // d^2 and R of one batch; the results of all P
    DevBuf<int32_t> d_centre;
    d_d.alloc((size_t)batch * nent);
    d_y.alloc((size_t)batch * nent);
    d_coeffs.alloc((size_t)P * ns);
    d_err.alloc(P);
    d_centre.alloc(P);
    struct Events {
        std::vector<hipEvent_t> e;
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    if (stage_ms) {
        ev.e.assign((size_t)3 * nbatch, nullptr);
        for (hipEvent_t &x : ev.e) MPSS_HIP(hipEventCreate(&x));
    }
    for (uint32_t b = 0; b < nbatch; ++b) {
        const uint32_t c0 = b * batch, nch = std::min(batch, P - c0);
        if (stage_ms) MPSS_HIP(hipEventRecord(ev.e[3 * b], st));
        fit_profiles_launch((int)c0, (int)nch, d_d.ptr, d_y.ptr, pw, st);
        if (stage_ms) MPSS_HIP(hipEventRecord(ev.e[3 * b + 1], st));
        // the fit reads the batch's d^2 and R where the profile stage left them: no wait, no copy
        sog_fit_launch(c0, nch, (uint32_t)nent, d_d.ptr, d_y.ptr, d_coeffs.ptr + (size_t)c0 * ns, d_err.ptr + c0,
                       d_centre.ptr + c0, fw, st);
        if (stage_ms) MPSS_HIP(hipEventRecord(ev.e[3 * b + 2], st));
    }
    std::vector<float> err(P);
    std::vector<int32_t> cen(P);
    MPSS_HIP(hipMemcpyAsync(coeffs, d_coeffs.ptr, sizeof(float) * (size_t)P * ns, hipMemcpyDeviceToHost, st));
    MPSS_HIP(hipMemcpyAsync(err.data(), d_err.ptr, sizeof(float) * P, hipMemcpyDeviceToHost, st));
    MPSS_HIP(hipMemcpyAsync(cen.data(), d_centre.ptr, sizeof(int32_t) * P, hipMemcpyDeviceToHost, st));
    MPSS_HIP(hipStreamSynchronize(st));
    if (stage_ms) {
        for (uint32_t b = 0; b < nbatch; ++b) {
            float ms = 0.f;
            MPSS_HIP(hipEventElapsedTime(&ms, ev.e[3 * b], ev.e[3 * b + 1]));
            stage_ms[0] += ms;
            MPSS_HIP(hipEventElapsedTime(&ms, ev.e[3 * b + 1], ev.e[3 * b + 2]));
            stage_ms[1] += ms;
        }
        stage_ms[2] = (double)pw.batches;
    }
    // (a centre of -1 here: every candidate's error was NaN)
    const int64_t bad = std::find_if(cen.begin(), cen.end(), [](int32_t c) { return c < 0; }) - cen.begin();
    fit_end(pl, err, cen, bad < (int64_t)P ? bad : -1, coeffs, error, centre, rgb);
}

void profile_fit_host(const mpss_profilefit &f, uint32_t *n_sigmas, uint32_t *n_ids, float *sigmas, float *coeffs,
                      float *error, float *rgb, int32_t *centre, uint32_t *length, float *pd, float *py) {
    FitPlan pl = make_fit_plan(f);
    if (length) *length = 0;
    if (!fit_begin(f, pl, "mpss_host_profile_fit", n_sigmas, n_ids, sigmas, coeffs)) return;
    const uint32_t ns = *n_sigmas, P = *n_ids * NB;
    const uint32_t L = (uint32_t)fit_profile_samples_host(f.desired_length);
    std::vector<float> dd((size_t)P * L), yy((size_t)P * L);
    {  // one profile per task over a few host threads (each profile is its own FFTs)
        std::atomic<uint32_t> next{0};
        std::atomic<bool> failed{false};
        std::vector<std::thread> th;
        const unsigned nt = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), P}));
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&] {
                std::vector<float> d, y;
                for (uint32_t p; (p = next.fetch_add(1)) < P;) {
                    try {
                        fit_channel_profile(pl.lp[p / NB], (int)(p % NB), f.desired_length, d, y);
                        if (d.size() != L) throw Error(MPSS_ERR_INTERNAL, "profile length");
                        memcpy(&dd[(size_t)p * L], d.data(), sizeof(float) * L);
                        memcpy(&yy[(size_t)p * L], y.data(), sizeof(float) * L);
                    } catch (...) {
                        failed = true;
                    }
                }
            });
        for (auto &x : th) x.join();
        if (failed) throw Error(MPSS_ERR_INTERNAL, "mpss_host_profile_fit: a host profile build failed");
    }
    if (length) *length = L;
    if (pd) memcpy(pd, dd.data(), sizeof(float) * dd.size());
    if (py) memcpy(py, yy.data(), sizeof(float) * yy.size());
    std::vector<float> err(P);
    std::vector<int32_t> cen(P);
    const int64_t bad = sog_fit_host(P, L, dd.data(), yy.data(), (int)ns, pl.sigmas.data(), pl.mfp_min.data(),
                                     pl.mfp_max.data(), coeffs, err.data(), cen.data(), nullptr, nullptr, nullptr);
    fit_end(pl, err, cen, bad, coeffs, error, centre, rgb);
}

}  // namespace mpss
