// pixel_sample.h -- a camera sample's values: the batch's replay table (reference-sampler mode)
// or the counter-hash sampler, for primary.hip and shade.hip.
#pragma once
#include "pbrt_math.h"
#include "render.h"

namespace mpss {

// Value k of camera sample s of pixel (px, py) in the batch's replay window (RenderScene::replay)
__device__ __forceinline__ float replay_val(const RenderScene &sc, int px, int py, int s, int k) {
    const int64_t p = (int64_t)(py - sc.replay_y0) * sc.replay_w + (px - sc.replay_x0);
    return sc.replay[((int64_t)k * sc.replay_npix + p) * sc.replay_spp + s];
}

// The image sample of camera sample s of pixel (px, py): LDPixelSample's imageX = xPos + u
__device__ __forceinline__ void image_sample(const RenderScene &sc, uint32_t seed, int px, int py, int s, float &X,
                                             float &Y) {
    if (sc.replay) {
        X = (float)px + replay_val(sc, px, py, s, 0);
        Y = (float)py + replay_val(sc, px, py, s, 1);
        return;
    }
    const uint32_t pix = (uint32_t)py * (uint32_t)sc.xres + (uint32_t)px;
    X = (float)px + van_der_corput((uint32_t)s, hash3(seed, pix, DIM_IMAGE));
    Y = (float)py + sobol2((uint32_t)s, hash3(seed, pix, DIM_IMAGE + 1));
}

}  // namespace mpss
