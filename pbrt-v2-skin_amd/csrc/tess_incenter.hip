// tess_incenter.hip -- tess_kernel's emitting pass with incentre points (tess_kernel.h).
#include "tess_kernel.h"

namespace mpss {

template __global__ void tess_kernel<true, true>(RenderScene, int, int, int64_t, float, int64_t *, const int64_t *,
                                                 SurfacePoint *);

}  // namespace mpss
