// pixel_filter.h -- the film's reconstruction filter: PixelFilter "box|triangle|gaussian|mitchell|sinc"
// (core/api.cpp:655-668 MakeFilter, filters/*.{h,cpp}), ImageFilm's 16 x 16 weight table
// (film/image.cpp:56-68), a sample's pixel range and table indices (AddSample, image.cpp:77-112), the
// film's sample extent (GetSampleExtent, image.cpp:157-166) and a tile's halo radius. Plain C++ (no
// HIP, no device pointers), so a CPU program can link pixel_filter.cpp alone (tests/pixel_filter_host);
// the per-sample routines are also compiled for the device (filter_pass.hip, film.hip).
#pragma once
#include <cmath>
#include <cstdint>

#include "tile_plan.h"

#if defined(__HIPCC__)
#define MPSS_PF_HD __host__ __device__ inline
#else
#define MPSS_PF_HD inline
#endif

namespace mpss {

// (the values of include/mpss.h MPSS_FILTER_*)
enum FilterKind { FILTER_BOX = 0, FILTER_TRIANGLE = 1, FILTER_GAUSSIAN = 2, FILTER_MITCHELL = 3, FILTER_SINC = 4 };
constexpr int kFilterKinds = 5;
constexpr int kFilterTableSize = 16;  // FILTER_TABLE_SIZE

// a, b: alpha (gaussian); B, C (mitchell); tau (sinc); unused otherwise
struct PixelFilter {
    int kind = FILTER_BOX;
    float xwidth = 0.5f, ywidth = 0.5f, a = 0.f, b = 0.f;
    // the filter film_kernel hard-codes: every weight 1, a one-pixel border, edge-rounded samples only
    bool is_default() const { return kind == FILTER_BOX && xwidth == 0.5f && ywidth == 0.5f; }
};

// The reference's defaults of `kind` (Create*Filter): box 0.5/0.5; triangle 2/2; gaussian 2/2 alpha 2;
// mitchell 2/2 B = C = 1/3; sinc 4/4 tau 3.
PixelFilter filter_defaults(int kind);
// Null when the description is usable, else what is wrong with it (unknown kind, width <= 0 or not
// finite or above kMaxFilterWidth, non-finite parameter).
const char *filter_invalid(const PixelFilter &f);
constexpr float kMaxFilterWidth = 32.f;
// Filter::Evaluate, in float, operation for operation
float filter_evaluate(const PixelFilter &f, float x, float y);
// filterTable: entry y * 16 + x = Evaluate((x + .5) xWidth / 16, (y + .5) yWidth / 16)
void filter_table(const PixelFilter &f, float table[kFilterTableSize * kFilterTableSize]);

// [xs, xe) x [ys, ye): the pixels whose samples the film wants (GetSampleExtent, no crop window)
struct SampleExtent {
    int xs, xe, ys, ye;
};
SampleExtent filter_sample_extent(const PixelFilter &f, int xres, int yres);
// Pixels a tile's samples are collected from beyond its edge, per axis: ceil(w + 0.5)
int filter_halo(float width);

// How the tile planner extends a tile's pieces (tile_plan.h): the default filter's one-pixel border inside
// the frame, which is what plan_tiles without a halo plans; any other filter's halo inside the sample extent.
PlanHalo filter_plan_halo(const PixelFilter &f, int xres, int yres);

// What the kernels need of a filter besides the table; a kernel argument.
struct FilterGeom {
    float wx, wy, inv_wx, inv_wy;  // Filter::xWidth, yWidth, invXWidth, invYWidth
    int rx, ry;                    // halo radius per axis
    int xs, xe, ys, ye;            // the sample extent
};
struct FilmFilter {
    FilterGeom g;
    float table[kFilterTableSize * kFilterTableSize];
};
FilmFilter film_filter(const PixelFilter &f, int xres, int yres);

// Pixel range [lo, hi] one image-sample coordinate reaches (AddSample: d = X - 0.5;
// [Ceil2Int(d - w), Floor2Int(d + w)] clamped to the res pixels of the frame); empty when hi < lo.
MPSS_PF_HD void filter_range(float X, float w, int res, int &lo, int &hi) {
    const float d = X - 0.5f;
    lo = (int)ceilf(d - w);
    hi = (int)floorf(d + w);
    lo = lo < 0 ? 0 : lo;
    hi = hi > res - 1 ? res - 1 : hi;
}
// ifx[x - x0] of AddSample: min(Floor2Int(fabsf((x - d) * invW * 16)), 15), d = X - 0.5
MPSS_PF_HD int filter_index(int x, float d, float inv_w) {
    const float fx = fabsf(((float)x - d) * inv_w * (float)kFilterTableSize);
    const int i = (int)floorf(fx);
    return i < kFilterTableSize - 1 ? i : kFilterTableSize - 1;
}
// The counter-hash sampler's key of pixel (px, py) of the sample extent: py * xres + px inside the
// frame (whatever the filter, so a frame keeps its camera samples when the filter changes); outside
// it that value would wrap onto an in-frame pixel, so those pixels are numbered after the frame in
// row-major order of the extent.
MPSS_PF_HD uint32_t filter_pixel_key(const FilterGeom &g, int xres, int yres, int px, int py) {
    if (px >= 0 && px < xres && py >= 0 && py < yres) return (uint32_t)py * (uint32_t)xres + (uint32_t)px;
    return (uint32_t)xres * (uint32_t)yres + (uint32_t)(py - g.ys) * (uint32_t)(g.xe - g.xs) + (uint32_t)(px - g.xs);
}
// ... and the pixel of a key (the inverse)
MPSS_PF_HD void filter_key_pixel(const FilterGeom &g, int xres, int yres, uint32_t key, int &px, int &py) {
    const uint32_t n = (uint32_t)xres * (uint32_t)yres;
    if (key < n) {
        px = (int)(key % (uint32_t)xres);
        py = (int)(key / (uint32_t)xres);
    } else {
        const uint32_t w = (uint32_t)(g.xe - g.xs);
        px = g.xs + (int)((key - n) % w);
        py = g.ys + (int)((key - n) / w);
    }
}

}  // namespace mpss
