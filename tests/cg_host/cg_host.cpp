// cg_host -- builds common grids with csrc/common_grid.cpp alone (no libmpss, no HIP runtime, no GPU), for
// tests/test_common_grid_sanitized.py to run under AddressSanitizer and UndefinedBehaviorSanitizer.
//
//   cg_host FILE...   each FILE: int32 L, int32 mode (0 runs of adjacent reach, 1 snake, 2 rgbprofile),
//                     float rcp[30], float table[30][L]
//
// Builds every file's grid for both LDS layouts as the library does (mpss_host_common_grid) and prints
// one line per grid. Exit 0 when all were built.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "common_grid.h"

using namespace mpss;

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        int32_t hdr[2];
        if (!f || fread(hdr, sizeof(int32_t), 2, f) != 2 || hdr[0] < 2) {
            fprintf(stderr, "cg_host: cannot read %s\n", argv[a]);
            return 2;
        }
        const int L = hdr[0], mode = hdr[1];
        std::vector<float> rcp(NB), tab((size_t)NB * L);
        const bool read = fread(rcp.data(), sizeof(float), NB, f) == (size_t)NB &&
                          fread(tab.data(), sizeof(float), tab.size(), f) == tab.size();
        fclose(f);
        if (!read) {
            fprintf(stderr, "cg_host: %s is short\n", argv[a]);
            return 2;
        }
        BandGroups g = make_band_groups(rcp.data(), mode == 1);
        if (mode == 2)
            for (int k = 0; k < kGroups; ++k)
                for (int j = 0; j < 4; ++j) g.band[k][j] = j < 3 ? j : -1;
        for (const int near_field : {5088, 10236}) {
            CommonGrid cg;
            std::vector<float4> rows;
            float rel[NB], l1[NB];
            const bool ok = build_common_grid(tab.data(), L, rcp.data(), g, cg, rows, rel, l1, near_field,
                                              mode == 2 ? 28 : 0, mode == 2);
            size_t flagged = 0;
            for (size_t r = 0; r < rows.size(); r += 2) flagged += rows[r].x != rows[r].x;
            float hmin = 1.f;
            for (int k = 0; k < kGroups; ++k) hmin = cg.hinv[k] < hmin ? cg.hinv[k] : hmin;
            printf("%s near_field %d ok %d rows %zu flagged %zu hinv_min %g\n", argv[a], near_field, ok ? 1 : 0,
                   rows.size() / 2, flagged, hmin);
        }
    }
    return 0;
}
