// thread_bvh on the CPU (tests/test_thread_bvh.py builds this with csrc/scene_plain.cpp alone, under ASan + UBSan).
// Reads trees from the file named on the command line, one per line:   n   nprims offset (n times)
// -- the pre-order skeleton of a linear BVH (nprims 0: interior, offset = second child) -- and prints the threaded
// copy's offsets as one JSON list per tree. A node whose other fields changed is an error (exit 2).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_plain.h"

using namespace mpss;

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: thread_bvh_host TREES\n");
        return 2;
    }
    int n;
    while (fscanf(f, "%d", &n) == 1) {
        std::vector<BvhNode> bvh((size_t)n);
        for (int i = 0; i < n; ++i) {
            int nprims, offset;
            if (fscanf(f, "%d %d", &nprims, &offset) != 2) {
                fprintf(stderr, "short tree\n");
                return 2;
            }
            BvhNode &b = bvh[i];
            for (int k = 0; k < 3; ++k) {
                b.bmin[k] = (float)(i - k);
                b.bmax[k] = (float)(i + k) + 0.5f;
            }
            b.offset = offset;
            b.nprims = (uint16_t)nprims;
            b.axis = (uint16_t)(i % 3);
        }
        const std::vector<BvhNode> th = thread_bvh(bvh);
        if (th.size() != bvh.size()) {
            fprintf(stderr, "size changed\n");
            return 2;
        }
        printf("[");
        for (int i = 0; i < n; ++i) {
            BvhNode want = bvh[i];
            if (want.nprims == 0) want.offset = th[i].offset;  // all an interior node may differ in
            if (memcmp(&want, &th[i], sizeof(BvhNode)) != 0) {
                fprintf(stderr, "node %d: a field other than an interior offset changed\n", i);
                return 2;
            }
            printf("%s%d", i ? "," : "", th[i].offset);
        }
        printf("]\n");
    }
    fclose(f);
    return 0;
}
