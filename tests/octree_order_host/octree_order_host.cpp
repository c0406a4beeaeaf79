// device_order on the CPU (tests/test_octree_device_order.py builds this with csrc/octree.cpp alone, under ASan +
// UBSan: host C++ only, no libmpss, no GPU). Reads point clouds from the file named on the command line:
//   n   then n times   x y z area black
// builds each with build_octree (normal +z; E of point i, band c = 1 + i + c / 64, or all zero for a black point) and
// prints one JSON object per cloud: the host tree ("flat") and device_order's copy ("dev"), each with its headers (16
// words per node), pt_hdr (4 words per slot), pt_e (ROW words per slot) and pt_index -- floats as their bit patterns.
#include <cstdio>
#include <cstring>
#include <vector>

#include "octree.h"

using namespace mpss;

static void words(const char *name, const void *p, size_t n, const char *end) {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w;
        memcpy(&w, (const char *)p + 4 * i, 4);
        printf("%s%u", i ? "," : "", w);
    }
    printf("]%s", end);
}

static void tree(const char *name, const std::vector<NodeHdr> &hdr, const std::vector<float> &pt_hdr,
                 const std::vector<float> &pt_e, const std::vector<int32_t> &pt_index, const char *end) {
    printf("\"%s\":{", name);
    words("hdr", hdr.data(), hdr.size() * 16, ",");
    words("pt_hdr", pt_hdr.data(), pt_hdr.size(), ",");
    words("pt_e", pt_e.data(), pt_e.size(), ",");
    words("pt_index", pt_index.data(), pt_index.size(), "");
    printf("}%s", end);
}

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: octree_order_host CLOUDS\n");
        return 2;
    }
    int n;
    while (fscanf(f, "%d", &n) == 1) {
        std::vector<float> P(3 * (size_t)n), N(3 * (size_t)n), E((size_t)n * NB), A((size_t)n);
        for (int i = 0; i < n; ++i) {
            int black;
            if (fscanf(f, "%f %f %f %f %d", &P[3 * i], &P[3 * i + 1], &P[3 * i + 2], &A[i], &black) != 5) {
                fprintf(stderr, "short cloud\n");
                return 2;
            }
            N[3 * i] = N[3 * i + 1] = 0.f;
            N[3 * i + 2] = 1.f;
            for (int c = 0; c < NB; ++c) E[(size_t)i * NB + c] = black ? 0.f : 1.f + (float)i + (float)c / 64.f;
        }
        FlatOctree t;
        build_octree(n, P.data(), N.data(), E.data(), A.data(), t);
        const DeviceOrder d = device_order(t);
        printf("{");
        tree("flat", t.hdr, t.pt_hdr, t.pt_e, t.pt_index, ",");
        tree("dev", d.hdr, d.pt_hdr, d.pt_e, d.pt_index, "");
        printf("}\n");
    }
    fclose(f);
    return 0;
}
