// film_filter.h -- the kernels of a render batch that exist only for a non-default pixel filter
// (pixel_filter.h): the camera pass and texture lookups over the pixels of the film's sample extent, and
// the table-weighted film. The default 0.5-wide box keeps primary_kernel, shade_tex_kernel and film_kernel.
#pragma once
#include "pixel_filter.h"
#include "render.h"

namespace mpss {

// film_filter_kernel: pixels per side of a workgroup's block, and the camera samples it stages in LDS
// at a time
constexpr int kFilmTile = 16, kFilmStage = 2048;

// image_sample (pixel_sample.h) of camera sample s of pixel (px, py) of the film's sample extent, `key`
// its filter_pixel_key: inside the frame, image_sample's values. Hash sampler only.
__device__ __forceinline__ void image_sample_keyed(uint32_t seed, uint32_t key, int px, int py, int s, float &X,
                                                   float &Y) {
    X = (float)px + van_der_corput((uint32_t)s, hash3(seed, key, DIM_IMAGE));
    Y = (float)py + sobol2((uint32_t)s, hash3(seed, key, DIM_IMAGE + 1));
}

__global__ void primary_filter_kernel(RenderScene sc, PieceList pl, SampleRecs rec0, FilterGeom fg);
__global__ void shade_tex_filter_kernel(RenderScene sc, SampleRecs rec, int spp, uint32_t seed, int max_hits,
                                        FilterGeom fg);
__global__ void shade_tex_filter_spec_kernel(RenderScene sc, SampleRecs rec, int spp, uint32_t seed, int max_hits,
                                        FilterGeom fg);
__global__ void film_filter_kernel(RenderScene sc, PieceList pl, SampleRecs rec0, FilmFilter f);

}  // namespace mpss
