// device_profile.cpp -- DeviceProfile's host side: the profile tables' upload and the common grids built
// from them (common_grid.h) for both LDS layouts of the sharded gather.
#include <algorithm>
#include <memory>
#include <thread>
#include <vector>

#include "common_grid.h"
#include "mo_kernel.h"
#include "spectral.h"

namespace mpss {

void DeviceProfile::upload(const float *tab, int len, const float *rcp_, bool snake, bool grid_host) {
    // two zero floats after the last band: the sharded gather's read for "past the profile end"
    const size_t n = (size_t)NB * len;
    if (table.n != n + 2) table.alloc(n + 2);
    MPSS_HIP(hipMemcpy(table.ptr, tab, n * sizeof(float), hipMemcpyHostToDevice));
    MPSS_HIP(hipMemset(table.ptr + n, 0, 2 * sizeof(float)));
    rcp.upload(rcp_, NB);
    L = len;
    rcp_min = rcp_[0];
    for (int c = 1; c < NB; ++c) rcp_min = rcp_[c] < rcp_min ? rcp_[c] : rcp_min;
    for (int c = 0; c < NB; ++c) host_rcp[c] = rcp_[c];
    groups = make_band_groups(rcp_, snake);
    rgb_refl.release();
    grid_on_host = grid_host;
    build_common(tab, groups, 0, false);
}

void DeviceProfile::set_rgb(const float *tab) {
    float refl[7][NB];
    for (int t = 0; t < 7; ++t) std::copy_n(rgb_refl2spect(t), NB, refl[t]);
    rgb_refl.upload(&refl[0][0], 7 * NB);
    // the common grid of the R, G, B profiles (rows 0..2, the same three slots in every group: the
    // sharded gather reads them in band_tree's lband order)
    BandGroups g3 = groups;
    for (int g = 0; g < kGroups; ++g)
        for (int j = 0; j < 4; ++j) g3.band[g][j] = j < 3 ? j : -1;
    build_common(tab, g3, 28, true);  // (the LDS's last 28 floats: the groups' FromRGB weights)
}

void DeviceProfile::build_common(const float *tab, const BandGroups &slots, int lds_reserve, bool rgb) {
    ctab.release();
    ctab_half.release();
    // the two LDS layouts' grids side by side (host work: each builds its groups on threads of its own)
    std::vector<float4> hh, h;
    bool ok_half = false;
    // the GPU builder: the per-knot scan of both layouts and all groups in one go, from the table
    // already on the device (the rgbprofile's rows 0..2 are the first rows of the same table)
    std::unique_ptr<CgScan[]> scan;
    if (!grid_on_host) {
        scan.reset(new CgScan[2]);
        if (!scan_common_grid_gpu(table.ptr, L, host_rcp, slots, lds_reserve, rgb, scan.get())) scan.reset();
    }
    std::thread half([&] {
        ok_half = build_common_grid(tab, L, host_rcp, slots, cg_half, hh, cg_rel_err[1], cg_l1_err[1], 5088,
                                    lds_reserve, rgb, scan ? &scan[1] : nullptr);
    });
    const bool ok = build_common_grid(tab, L, host_rcp, slots, cg, h, cg_rel_err[0], cg_l1_err[0], 10236,
                                      lds_reserve, rgb, scan ? &scan[0] : nullptr);
    half.join();
    if (ok_half) {
        ctab_half.upload(hh.data(), hh.size());
        cg_half.tab = ctab_half.ptr;
    } else {
        cg_half.on = 0;
    }
    if (!ok) {
        cg.on = 0;  // the per-band tables stay in use
        return;
    }
    ctab.upload(h.data(), h.size());
    cg.tab = ctab.ptr;
}

}  // namespace mpss
