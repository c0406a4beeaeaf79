// film_spectral.h -- the kernels of a render batch that exist only for a spectral call
// (mpss_render_tile_spectral): after assemble_kernel<true> / sky_kernel<true> (film.hip) have left every
// sample's 30-band L in its hit's Ld row (zeros for a rejected sample), the films of those rows
// (film_spectral.hip). An XYZ call keeps the kernels it always ran.
#pragma once
#include "film_filter.h"
#include "render.h"

namespace mpss {

// The spectral films give a pixel kSpecLanes adjacent lanes, 4 bands a lane; the filtered film's workgroup
// owns kSpecTileX x kSpecTileY pixels. out[k] of their PieceList: a piece's rows of ROW floats per pixel.
constexpr int kSpecLanes = 8, kSpecTileX = 8, kSpecTileY = 4;
static_assert(kSpecLanes * 4 == ROW && kSpecLanes * kSpecTileX * kSpecTileY == 256, "a pixel's row over its lanes");

__global__ void film_spectral_kernel(RenderScene sc, PieceList pl, SampleRecs rec0);
__global__ void film_filter_spectral_kernel(RenderScene sc, PieceList pl, SampleRecs rec0, FilmFilter f);

}  // namespace mpss
