// tess_centroid.hip -- tess_kernel's counting pass and its emitting pass with centroid points
// (TessellateSurfacePoints, surfacepoints.cpp:328-332): Preprocess, before any render batch.
#include "tess_kernel.h"

namespace mpss {

template __global__ void tess_kernel<false, false>(RenderScene, int, int, int64_t, float, int64_t *, const int64_t *,
                                                   SurfacePoint *);
template __global__ void tess_kernel<true, false>(RenderScene, int, int, int64_t, float, int64_t *, const int64_t *,
                                                  SurfacePoint *);

}  // namespace mpss
