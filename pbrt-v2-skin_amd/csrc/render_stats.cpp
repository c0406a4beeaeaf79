// render_stats.cpp -- instrumentation of the per-pixel path: the event pairs around its timed kernels
// (cfg_.kernel_timing) and the gather's traversal counters (cfg_.count_traversal), as mpss_render_stats.
#include "context.h"

namespace mpss {

void Context::time_begin(bool on, hipStream_t s, hipEvent_t &a) {
    if (!on) return;
    MPSS_HIP(hipEventCreate(&a));
    MPSS_HIP(hipEventRecord(a, s));
}

void Context::time_end(bool on, hipStream_t s, hipEvent_t a, int kind, std::vector<Timed> &out) {
    if (!on) return;
    hipEvent_t b;
    MPSS_HIP(hipEventCreate(&b));
    MPSS_HIP(hipEventRecord(b, s));
    out.push_back(Timed{a, b, kind});
}

mpss_render_stats Context::render_stats() {
    activate();
    std::lock_guard<std::mutex> g(mu_);
    MPSS_HIP(hipDeviceSynchronize());
    for (const Timed &t : timed_) {
        float ms = 0.f;
        MPSS_HIP(hipEventElapsedTime(&ms, t.a, t.b));
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
        double *dst[7] = {&stats_.ms_irradiance, &stats_.ms_camera, &stats_.ms_shade, &stats_.ms_film,
                          &stats_.ms_direct, &stats_.ms_tex, &stats_.ms_replay};
        int64_t *cnt[7] = {&stats_.n_irradiance, &stats_.n_camera, &stats_.n_shade, &stats_.n_film, &stats_.n_direct,
                           &stats_.n_tex, &stats_.n_replay};
        *dst[t.kind] += ms;
        *cnt[t.kind] += 1;
    }
    timed_.clear();
    mpss_render_stats out = stats_;
    const int sm = first_bssrdf_material();
    for (int g2 = 0; g2 < kGroups; ++g2)
        for (int s = 0; s < 4; ++s)
            out.group_bands[g2][s] = sm >= 0 ? materials_[sm]->dev_profile.groups.band[g2][s] : -1;
    if (d_counts_.ptr) {
        unsigned long long c[kStatStride * kGroups];
        MPSS_HIP(hipMemcpy(c, d_counts_.ptr, sizeof(c), hipMemcpyDeviceToHost));
        for (int g2 = 0; g2 < kGroups; ++g2) {
            out.mo_nodes += (int64_t)c[kStatStride * g2];
            out.mo_points += (int64_t)c[kStatStride * g2 + 1];
            out.group_nodes[g2] = (int64_t)c[kStatStride * g2];
            out.group_points[g2] = (int64_t)c[kStatStride * g2 + 1];
            out.mo_wave_node_iters += (int64_t)c[kStatStride * g2 + 2];
            out.mo_wave_point_iters += (int64_t)c[kStatStride * g2 + 3];
            out.mo_lookups += (int64_t)c[kStatStride * g2 + 4];
            for (int k = 0; k < 3; ++k) out.mo_lookups_near[k] += (int64_t)c[kStatStride * g2 + 5 + k];
            out.mo_row_lane_records += (int64_t)c[kStatStride * g2 + 8];
            out.mo_lds_lane_records += (int64_t)c[kStatStride * g2 + 9];
            out.mo_table_lane_records += (int64_t)c[kStatStride * g2 + 10];
            for (int k = 0; k < 3; ++k) out.group_path_records[g2][k] = (int64_t)c[kStatStride * g2 + 8 + k];
            for (int k = 0; k < 2; ++k) {
                out.group_path_sectors[g2][k] = (int64_t)c[kStatStride * g2 + 11 + k];
                out.group_path_lines[g2][k] = (int64_t)c[kStatStride * g2 + 13 + k];
                out.group_path_fetches[g2][k] = (int64_t)c[kStatStride * g2 + 15 + k];
            }
        }
    }
    return out;
}

void Context::reset_render_stats() {
    (void)render_stats();  // drain pending events
    std::lock_guard<std::mutex> g(mu_);
    stats_ = mpss_render_stats{};
    if (d_counts_.ptr) MPSS_HIP(hipMemset(d_counts_.ptr, 0, kStatStride * kGroups * sizeof(unsigned long long)));
}

int Context::first_bssrdf_material() const {
    for (size_t i = 0; i < materials_.size(); ++i)
        if (!materials_[i]->dipole && !materials_[i]->no_bssrdf) return (int)i;
    return -1;
}

}  // namespace mpss
