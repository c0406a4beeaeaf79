// spectrum_tables.h -- the 30-band spectrum on the device: the CIE matching curves, the RGB ->
// spectrum uplift of SampledSpectrum::FromRGB (spectrum.cpp:103-187) with its tables, Pow(albedo, e)
// of a textured albedo, and the rho_hd lookup. Every unit that includes this carries its own copy of
// the __constant__ tables (a few KB).
#pragma once
#include "../../data/spectral_bands.h"
#include "common.h"
#include "pbrt_math.h"
#include "texture.h"

namespace mpss {
namespace {

__constant__ float kCieX[NB] = MPSS_BAND_CIE_X_INIT;
__constant__ float kCieY[NB] = MPSS_BAND_CIE_Y_INIT;
__constant__ float kCieZ[NB] = MPSS_BAND_CIE_Z_INIT;
// rgbIllum2Spect{White, Cyan, Magenta, Yellow, Red, Green, Blue} (spectrum.cpp:316-370)
__constant__ float kIllum[7][NB] = {MPSS_BAND_RGBILLUM2SPECTWHITE_INIT,  MPSS_BAND_RGBILLUM2SPECTCYAN_INIT,
                                    MPSS_BAND_RGBILLUM2SPECTMAGENTA_INIT, MPSS_BAND_RGBILLUM2SPECTYELLOW_INIT,
                                    MPSS_BAND_RGBILLUM2SPECTRED_INIT,     MPSS_BAND_RGBILLUM2SPECTGREEN_INIT,
                                    MPSS_BAND_RGBILLUM2SPECTBLUE_INIT};

// rgbRefl2Spect{White, Cyan, Magenta, Yellow, Red, Green, Blue} (spectrum.cpp:316-370)
__constant__ float kRefl[7][NB] = {MPSS_BAND_RGBREFL2SPECTWHITE_INIT,  MPSS_BAND_RGBREFL2SPECTCYAN_INIT,
                                   MPSS_BAND_RGBREFL2SPECTMAGENTA_INIT, MPSS_BAND_RGBREFL2SPECTYELLOW_INIT,
                                   MPSS_BAND_RGBREFL2SPECTRED_INIT,     MPSS_BAND_RGBREFL2SPECTGREEN_INIT,
                                   MPSS_BAND_RGBREFL2SPECTBLUE_INIT};

// band c of Spectrum(rgb, SPECTRUM_ILLUMINANT) = SampledSpectrum::FromRGB (spectrum.cpp:103-187)
__device__ __forceinline__ float illum_band(const float rgb[3], int c) {
    const float R = rgb[0], G = rgb[1], B = rgb[2];
    float r = 0.f;
    if (R <= G && R <= B) {
        r += kIllum[0][c] * R;
        if (G <= B) {
            r += kIllum[1][c] * (G - R);
            r += kIllum[6][c] * (B - G);
        } else {
            r += kIllum[1][c] * (B - R);
            r += kIllum[5][c] * (G - B);
        }
    } else if (G <= R && G <= B) {
        r += kIllum[0][c] * G;
        if (R <= B) {
            r += kIllum[2][c] * (R - G);
            r += kIllum[6][c] * (B - R);
        } else {
            r += kIllum[2][c] * (B - G);
            r += kIllum[4][c] * (R - B);
        }
    } else {
        r += kIllum[0][c] * B;
        if (R <= G) {
            r += kIllum[3][c] * (R - B);
            r += kIllum[5][c] * (G - R);
        } else {
            r += kIllum[3][c] * (G - B);
            r += kIllum[4][c] * (R - G);
        }
    }
    const float v = r * .86445f;
    return v < 0.f ? 0.f : v;  // Clamp(0, INFINITY)
}

// band c of Spectrum::FromRGB(rgb) (reflectance; spectrum.cpp:103-187): ImageTexture's convertOut.
// Its six cases stand three times in this file: here, in tex_albedo_pow_all and in refl_split (with
// refl_split_band). A change to the rows or the order of one is a change to all three.
__device__ __forceinline__ float refl_band(const float rgb[3], int c) {
    const float R = rgb[0], G = rgb[1], B = rgb[2];
    float r = 0.f;
    if (R <= G && R <= B) {
        r += kRefl[0][c] * R;
        if (G <= B) {
            r += kRefl[1][c] * (G - R);
            r += kRefl[6][c] * (B - G);
        } else {
            r += kRefl[1][c] * (B - R);
            r += kRefl[5][c] * (G - B);
        }
    } else if (G <= R && G <= B) {
        r += kRefl[0][c] * G;
        if (R <= B) {
            r += kRefl[2][c] * (R - G);
            r += kRefl[6][c] * (B - R);
        } else {
            r += kRefl[2][c] * (B - G);
            r += kRefl[4][c] * (R - B);
        }
    } else {
        r += kRefl[0][c] * B;
        if (R <= G) {
            r += kRefl[3][c] * (R - B);
            r += kRefl[5][c] * (G - R);
        } else {
            r += kRefl[3][c] * (G - B);
            r += kRefl[4][c] * (R - G);
        }
    }
    const float v = r * .94f;
    return v < 0.f ? 0.f : v;
}

// Pow(albedo, e) band c for a textured albedo: the ImageTexture value at the point, FromRGB. The
// exponent is mix or 1 - mix, 0.5 at the default mix: then pow(x, 0.5) = sqrt(x) for every x >= +0
// (refl_band clamps at 0) -- the correctly rounded sqrtf, where the double pow rounded to float costs
// a software log and exp per band per hit (3.3 ms of a textured C2 frame's 3.4 M SSS hits x 30 bands)
__device__ __noinline__ float tex_pow_general(float x, float e) { return m_pow(x, e); }
__device__ __forceinline__ float tex_albedo_pow(const float rgb[3], int c, float e) {
    const float x = refl_band(rgb, c);
    return e == 0.5f ? __builtin_sqrtf(x) : tex_pow_general(x, e);
}

// Pow(FromRGB(rgb), e) for all 30 bands of a textured albedo, the branches of refl_band (FromRGB,
// spectrum.cpp:103-187) decided once per lane instead of per band: the minimum / middle / maximum
// components and the rows of their secondary (X: Cyan, Magenta, Yellow) and primary (Y: Red, Green,
// Blue) spectra; then per band the same products and sums in the same order. e = 0.5 (the default mix)
// as sqrtf (tex_albedo_pow). (The case table is refl_band's and refl_split's: keep the three alike.)
__device__ __forceinline__ void tex_albedo_pow_all(const float4 rgb, float e, float out[NB]) {
    const float R = rgb.x, G = rgb.y, B = rgb.z;
    float mn, md, mx;
    int xi, yi;
    if (R <= G && R <= B) {
        mn = R;
        xi = 1;
        if (G <= B) { md = G; mx = B; yi = 6; } else { md = B; mx = G; yi = 5; }
    } else if (G <= R && G <= B) {
        mn = G;
        xi = 2;
        if (R <= B) { md = R; mx = B; yi = 6; } else { md = B; mx = R; yi = 4; }
    } else {
        mn = B;
        xi = 3;
        if (R <= G) { md = R; mx = G; yi = 5; } else { md = G; mx = R; yi = 4; }
    }
    const float d1 = md - mn, d2 = mx - md;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const float X = xi == 1 ? kRefl[1][c] : (xi == 2 ? kRefl[2][c] : kRefl[3][c]);
        const float Y = yi == 4 ? kRefl[4][c] : (yi == 5 ? kRefl[5][c] : kRefl[6][c]);
        float r = 0.f;
        r += kRefl[0][c] * mn;
        r += X * d1;
        r += Y * d2;
        float v = r * .94f;
        v = v < 0.f ? 0.f : v;
        out[c] = e == 0.5f ? __builtin_sqrtf(v) : tex_pow_general(v, e);
    }
}

// FromRGB(rgb) (reflectance) with refl_band's branches decided once, for a spectrum that is read band by
// band later (a hit's Kr / Kt texture lookup, shade.hip): the minimum component, the two differences and
// the rows of the secondary and primary spectra, as tex_albedo_pow_all picks them; refl_split_band(s, c)
// is refl_band(rgb, c) -- the same products and sums in the same order. (The case table is refl_band's
// and tex_albedo_pow_all's: keep the three alike; test_spec_texture_gpu's block textures hold this copy
// to the oracle's FromRGB in each of its colours' cases.)
struct ReflSplit {
    float mn, d1, d2;
    int xi, yi;
};
__device__ __forceinline__ ReflSplit refl_split(float R, float G, float B) {
    float mn, md, mx;
    int xi, yi;
    if (R <= G && R <= B) {
        mn = R;
        xi = 1;
        if (G <= B) { md = G; mx = B; yi = 6; } else { md = B; mx = G; yi = 5; }
    } else if (G <= R && G <= B) {
        mn = G;
        xi = 2;
        if (R <= B) { md = R; mx = B; yi = 6; } else { md = B; mx = R; yi = 4; }
    } else {
        mn = B;
        xi = 3;
        if (R <= G) { md = R; mx = G; yi = 5; } else { md = G; mx = R; yi = 4; }
    }
    return ReflSplit{mn, md - mn, mx - md, xi, yi};
}
__device__ __forceinline__ float refl_split_band(const ReflSplit &s, int c) {
    const float X = s.xi == 1 ? kRefl[1][c] : (s.xi == 2 ? kRefl[2][c] : kRefl[3][c]);
    const float Y = s.yi == 4 ? kRefl[4][c] : (s.yi == 5 ? kRefl[5][c] : kRefl[6][c]);
    float r = 0.f;
    r += kRefl[0][c] * s.mn;
    r += X * s.d1;
    r += Y * s.d2;
    const float v = r * .94f;
    return v < 0.f ? 0.f : v;
}

// A hit's Kr / Kt record (SampleRecs::hit_kr, hit_kt): the texture's RGB at the hit's shading geometry and,
// in w, whether FromRGB of it has a nonzero band (!Spectrum::IsBlack(): 1, else 0)
__device__ __forceinline__ float4 spec_lookup(const TexView &T, const UVDiff &g) {
    float rgb[3];
    tex_eval(T, g, rgb);
    const ReflSplit s = refl_split(rgb[0], rgb[1], rgb[2]);
    bool black = true;
    for (int c = 0; c < NB; ++c) black = black && refl_split_band(s, c) == 0.f;
    return make_float4(rgb[0], rgb[1], rgb[2], black ? 0.f : 1.f);
}

__device__ __forceinline__ float rho_lookup(const float *hd, int n, float ct) {  // multipole.cpp:458-463
    const float fid = ct * (float)(n - 1);
    int id = (int)fid;
    id = id < 0 ? 0 : (id > n - 2 ? n - 2 : id);
    const float t = fid - (float)id;
    return (1.f - t) * hd[id] + t * hd[id + 1];
}

}  // namespace
}  // namespace mpss
