// The Poisson-disk acceptance on the CPU (tests/test_poisson_accept.py builds this with csrc/poisson_accept.cpp
// alone, under ASan + UBSan). Reads cases from the file named on the command line. A case is
//   min_dist max_fails area batch batches stride nlaunch        (floats as their uint32 bit patterns)
// followed, per launch, by   npaths   and npaths times   i cnt  x y z (cnt times):
// path i of the launch (0 <= i < batch * batches, ascending) has cnt <= stride candidates at those positions;
// every other path has none. Candidates are numbered in file order from 0 (their SurfacePoint::material).
// The launches are fed to one PoissonAccept while it says GoOn. One JSON line per case:
//   {"accepted": [candidate numbers], "state": "go_on" | "done" | "gave_up", "repeated_fails": n,
//    "total_paths": n, "launches": launches consumed}
// An accepted point that is not its candidate with area replaced is an error (exit 2).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poisson_accept.h"

using namespace mpss;

static float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, sizeof(f));
    return f;
}

static void fail(const char *what) {
    fprintf(stderr, "poisson_accept_host: %s\n", what);
    exit(2);
}

int main(int argc, char **argv) {
    if (argc != 2) fail("usage: poisson_accept_host CASES");
    FILE *f = fopen(argv[1], "r");
    if (!f) fail("cannot open the case file");
    uint32_t md_bits, area_bits;
    int max_fails, batch, batches, stride, nlaunch;
    while (fscanf(f, "%u %d %u %d %d %d %d", &md_bits, &max_fails, &area_bits, &batch, &batches, &stride, &nlaunch) == 7) {
        const float area = from_bits(area_bits);
        PoissonAccept acc(from_bits(md_bits), max_fails, area);
        PoissonAccept::State state = PoissonAccept::State::GoOn;
        std::vector<SurfacePoint> all;  // by candidate number
        int used = 0;
        for (int l = 0; l < nlaunch; ++l) {
            // a launch's arrays are its own, exactly sized: a read outside them is the sanitizer's to report
            std::vector<int> cnt((size_t)batch * batches, 0);
            SurfacePoint poison;
            memset(&poison, 0xff, sizeof(poison));  // (NaN coordinates)
            std::vector<SurfacePoint> cand((size_t)batch * batches * stride, poison);
            int npaths;
            if (fscanf(f, "%d", &npaths) != 1) fail("short case");
            for (int k = 0; k < npaths; ++k) {
                int i, c;
                if (fscanf(f, "%d %d", &i, &c) != 2 || i < 0 || i >= batch * batches || c < 0 || c > stride)
                    fail("bad path");
                cnt[i] = c;
                for (int j = 0; j < c; ++j) {
                    uint32_t b[3];
                    if (fscanf(f, "%u %u %u", &b[0], &b[1], &b[2]) != 3) fail("short path");
                    SurfacePoint sp{};
                    for (int a = 0; a < 3; ++a) sp.p[a] = from_bits(b[a]);
                    sp.material = (uint32_t)all.size();
                    sp.n[2] = 1.f;
                    sp.u = 0.25f + (float)all.size();
                    sp.v = 0.5f;
                    sp.area = -1.f;
                    sp.ray_eps = 1e-3f;
                    all.push_back(sp);
                    cand[(size_t)i * stride + j] = sp;
                }
            }
            if (state != PoissonAccept::State::GoOn) continue;  // (the rest of the case is read, not fed)
            state = acc.consume(cand.data(), cnt.data(), batch, batches, stride);
            ++used;
        }
        printf("{\"accepted\":[");
        for (size_t k = 0; k < acc.points.size(); ++k) {
            const SurfacePoint &p = acc.points[k];
            if (p.material >= all.size()) fail("an accepted point that is no candidate");
            SurfacePoint want = all[p.material];
            want.area = area;
            if (memcmp(&want, &p, sizeof(p)) != 0) fail("an accepted point differs from its candidate");
            printf("%s%u", k ? "," : "", p.material);
        }
        printf("],\"state\":\"%s\",\"repeated_fails\":%d,\"total_paths\":%lld,\"launches\":%d}\n",
               state == PoissonAccept::State::GoOn ? "go_on" : state == PoissonAccept::State::Done ? "done" : "gave_up",
               acc.repeated_fails, (long long)acc.total_paths, used);
    }
    fclose(f);
    return 0;
}
