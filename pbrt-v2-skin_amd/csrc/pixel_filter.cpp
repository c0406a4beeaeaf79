// pixel_filter.cpp -- the reconstruction filters and ImageFilm's weight table (pixel_filter.h).
#include "pixel_filter.h"

#include <algorithm>

namespace mpss {

PixelFilter filter_defaults(int kind) {
    PixelFilter f;
    f.kind = kind;
    switch (kind) {
    case FILTER_TRIANGLE: f.xwidth = f.ywidth = 2.f; break;
    case FILTER_GAUSSIAN: f.xwidth = f.ywidth = 2.f; f.a = 2.f; break;
    case FILTER_MITCHELL: f.xwidth = f.ywidth = 2.f; f.a = f.b = 1.f / 3.f; break;
    case FILTER_SINC: f.xwidth = f.ywidth = 4.f; f.a = 3.f; break;
    default: f.xwidth = f.ywidth = 0.5f; break;
    }
    return f;
}

const char *filter_invalid(const PixelFilter &f) {
    if (f.kind < 0 || f.kind >= kFilterKinds) return "unknown filter kind";
    if (!(f.xwidth > 0.f) || !(f.ywidth > 0.f) || !std::isfinite(f.xwidth) || !std::isfinite(f.ywidth))
        return "filter widths must be positive and finite";
    if (f.xwidth > kMaxFilterWidth || f.ywidth > kMaxFilterWidth) return "filter widths must be at most 32 pixels";
    if (!std::isfinite(f.a) || !std::isfinite(f.b)) return "filter parameters must be finite";
    return nullptr;
}

namespace {

// GaussianFilter::Gaussian (filters/gaussian.h)
float gaussian1d(float alpha, float d, float expv) { return std::max(0.f, float(expf(-alpha * d * d) - expv)); }

// MitchellFilter::Mitchell1D (filters/mitchell.h)
float mitchell1d(float B, float C, float x) {
    x = fabsf(2.f * x);
    if (x > 1.f)
        return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) *
               (1.f / 6.f);
    else
        return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) * (1.f / 6.f);
}

// LanczosSincFilter::Sinc1D (filters/sinc.h): the comparisons and the product with pi are in double
float sinc1d(float tau, float x) {
    x = fabsf(x);
    if (x < 1e-5) return 1.f;
    if (x > 1.) return 0.f;
    x *= 3.14159265358979323846;
    const float sinc = sinf(x) / x;
    const float lanczos = sinf(x * tau) / (x * tau);
    return sinc * lanczos;
}

}  // namespace

float filter_evaluate(const PixelFilter &f, float x, float y) {
    switch (f.kind) {
    case FILTER_TRIANGLE: return std::max(0.f, f.xwidth - fabsf(x)) * std::max(0.f, f.ywidth - fabsf(y));
    case FILTER_GAUSSIAN: {
        const float expX = expf(-f.a * f.xwidth * f.xwidth), expY = expf(-f.a * f.ywidth * f.ywidth);
        return gaussian1d(f.a, x, expX) * gaussian1d(f.a, y, expY);
    }
    case FILTER_MITCHELL: return mitchell1d(f.a, f.b, x * (1.f / f.xwidth)) * mitchell1d(f.a, f.b, y * (1.f / f.ywidth));
    case FILTER_SINC: return sinc1d(f.a, x * (1.f / f.xwidth)) * sinc1d(f.a, y * (1.f / f.ywidth));
    default: return 1.f;
    }
}

void filter_table(const PixelFilter &f, float table[kFilterTableSize * kFilterTableSize]) {
    float *ftp = table;
    for (int y = 0; y < kFilterTableSize; ++y) {
        const float fy = ((float)y + .5f) * f.ywidth / kFilterTableSize;
        for (int x = 0; x < kFilterTableSize; ++x) {
            const float fx = ((float)x + .5f) * f.xwidth / kFilterTableSize;
            *ftp++ = filter_evaluate(f, fx, fy);
        }
    }
}

SampleExtent filter_sample_extent(const PixelFilter &f, int xres, int yres) {
    SampleExtent e;
    e.xs = (int)floorf(0 + 0.5f - f.xwidth);
    e.xe = (int)ceilf(0 + 0.5f + xres + f.xwidth);
    e.ys = (int)floorf(0 + 0.5f - f.ywidth);
    e.ye = (int)ceilf(0 + 0.5f + yres + f.ywidth);
    return e;
}

int filter_halo(float width) { return (int)ceilf(width + 0.5f); }

PlanHalo filter_plan_halo(const PixelFilter &f, int xres, int yres) {
    if (f.is_default()) return PlanHalo{1, 1, 0, xres, 0, yres};
    const SampleExtent e = filter_sample_extent(f, xres, yres);
    return PlanHalo{filter_halo(f.xwidth), filter_halo(f.ywidth), e.xs, e.xe, e.ys, e.ye};
}

FilmFilter film_filter(const PixelFilter &f, int xres, int yres) {
    FilmFilter ff;
    const SampleExtent e = filter_sample_extent(f, xres, yres);
    ff.g = FilterGeom{f.xwidth, f.ywidth, 1.f / f.xwidth, 1.f / f.ywidth, filter_halo(f.xwidth), filter_halo(f.ywidth),
                      e.xs,     e.xe,     e.ys,           e.ye};
    filter_table(f, ff.table);
    return ff;
}

}  // namespace mpss
