// scene_plain.cpp -- thread_bvh (scene_plain.h): plain C++, linked alone by tests/thread_bvh_host.
#include "scene_plain.h"

namespace mpss {

std::vector<BvhNode> thread_bvh(const std::vector<BvhNode> &bvh) {
    std::vector<BvhNode> th = bvh;
    std::vector<int32_t> end(th.size());
    for (size_t i = th.size(); i-- > 0;)
        end[i] = th[i].nprims > 0 ? (int32_t)i + 1 : end[th[i].offset];
    for (size_t i = 0; i < th.size(); ++i)
        if (th[i].nprims == 0) th[i].offset = end[i];
    return th;
}

}  // namespace mpss
