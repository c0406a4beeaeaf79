// film.hip -- steps 4 and 5 of a render batch (DESIGN.md "A render batch"), after the Mo() gather:
//   assemble_kernel  Li assembly (multipolesubsurface.cpp:253-303: L = Le + SSS + Ld), the
//                    NaN/negative/inf sample filter (samplerrenderer.cpp:119-133) and ToXYZ
//   sky_kernel       the same for camera rays that escaped to infinite lights (samplerrenderer.cpp:144-151)
//   film_kernel      ImageFilm::AddSample with the 0.5-wide box filter (film/image.cpp:77-137)
//   film_filter_kernel  ... with any other filter, through ImageFilm's weight table (pixel_filter.h)
// A spectral call (mpss_render_tile_spectral) runs the <true> instances of the first two, which also leave the
// sample's 30-band L in the hit's own Ld row (zeros for a sample the filter rejects); the films over those
// rows are film_spectral.hip's.
#include "render.h"

#include "film_filter.h"
#include "geom.h"
#include "light_sample.h"
#include "spectrum_tables.h"

namespace mpss {

// ------------------------------------------------------------------ film
// Li of one camera sample with radiance (MultipoleSubsurfaceIntegrator::Li,
// multipolesubsurface.cpp:253-303): L = 0 + Le; L += ((INV_PI * Ft) * Mo * Pow(albedo, 1 - mix))
// .Clamp(0); L += Ld -- then the SamplerRenderer sample filter (NaN / y < -1e-5 / inf -> 0,
// samplerrenderer.cpp:119-133) and Spectrum::ToXYZ in band order. One lane per slot.
// The common wave: every lane an SSS hit of one untextured material. The material is then
// wave-uniform (its tables are scalar loads), the lane's Ld row and the band-ordered Mo() values
// are all issued up front, and the 30-band loop is unrolled -- the same float operations, in the
// same order, as the general path below.
template <bool TEX, bool SPEC>
__device__ __forceinline__ void assemble_uniform(const RenderScene &sc, const SampleRecs &rec, int slot, int mid) {
    const RenderMaterial &mat = sc.materials[mid];
    const float4 q = rec.hit_q[slot];
    const float Ft = mat.is_mc ? 1.f : 1.f - rho_lookup(mat.rho, mat.n_rho, q.w);
    const float kss = kInvPiF * Ft;
    const float *mo = reinterpret_cast<const float *>(rec.mo4 + (size_t)slot * kGroups);
    const float4 *ld4 = reinterpret_cast<const float4 *>(rec.ld + (size_t)slot * ROW);
    float ld[32], m[NB];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 v = ld4[k];
        ld[4 * k] = v.x;
        ld[4 * k + 1] = v.y;
        ld[4 * k + 2] = v.z;
        ld[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) m[c] = mo[mat.band_pos[c]];
    float ab[NB];
    if (TEX) {  // the hit's albedo texture value (shade_tex_kernel): Pow(albedo, 1 - mix) per lane
        tex_albedo_pow_all(rec.hit_alb[slot], 1.f - mat.mix, ab);
    } else {
#pragma unroll
        for (int c = 0; c < NB; ++c) ab[c] = mat.alb_1mmix[c];
    }
    float X = 0.f, Y = 0.f, Z = 0.f;
    bool nan = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        float L = 0.f;
        float t = (kss * m[c]) * ab[c];
        t = t < 0.f ? 0.f : t;  // Spectrum::Clamp(0, INFINITY)
        L += t;
        L += ld[c];
        nan = nan || (L != L);
        X += kCieX[c] * L;
        Y += kCieY[c] * L;
        Z += kCieZ[c] * L;
        if (SPEC) ld[c] = L;
    }
    const float scale = (float)(700 - 400) / (float)(MPSS_CIE_Y_INTEGRAL * NB);
    const float y = Y * (float)(700 - 400) / (float)(MPSS_CIE_Y_INTEGRAL * NB);
    X *= scale;
    Y *= scale;
    Z *= scale;
    if (nan || y < -1e-5f || __builtin_isinf(y)) X = Y = Z = 0.f;
    rec.xyz[slot] = make_float4(X, Y, Z, 0.f);
    if (SPEC) {  // the sample's L over its Ld row (read above), 0 for a rejected sample
        const bool rej = nan || y < -1e-5f || __builtin_isinf(y);
        float4 *row = reinterpret_cast<float4 *>(rec.ld + (size_t)slot * ROW);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            row[k] = rej ? make_float4(0.f, 0.f, 0.f, 0.f)
                         : make_float4(ld[4 * k], ld[4 * k + 1], ld[4 * k + 2], ld[4 * k + 3]);
    }
}

// SPEC (a spectral call): the sample's L also goes over the hit's Ld row, 0 for a rejected sample
template <bool SPEC>
__global__ __launch_bounds__(256) void assemble_kernel(RenderScene sc, SampleRecs rec, int max_hits) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int nhits = *rec.hit_count;
    const bool in = slot < nhits && slot < max_hits;
    {
        const uint32_t hs0 = in ? rec.hit_s[slot] : 0u;
        const int mid = (int)((hs0 >> REC_MAT_SHIFT) & 0xffu);
        const int mid0 = __builtin_amdgcn_readfirstlane(mid);
        // SSS hit (bit 31, not a light) of material mid0 (with or without an albedo texture)
        const bool fast = in && (hs0 >> 31) && mid == mid0;
        if (__builtin_amdgcn_ballot_w64(in && !fast) == 0) {
            if (in) {
                if (sc.materials[mid0].has_alb_tex)
                    assemble_uniform<true, SPEC>(sc, rec, slot, mid0);
                else
                    assemble_uniform<false, SPEC>(sc, rec, slot, mid0);
            }
            return;
        }
    }
    if (!in) return;
    const uint32_t hs = rec.hit_s[slot];
    const float *le = nullptr, *mo = nullptr, *ld = nullptr;
    const RenderMaterial *mat = nullptr;
    float kss = 0.f, arg[3] = {0.f, 0.f, 0.f};
    bool alb = false;
    if ((hs & HS_LIGHT) && !(hs & HS_LSURF)) return;  // escaped: sky_kernel
    if (hs & HS_LIGHT) {  // a light sphere: L = 0 + Le(wo) (if it faces the ray) + Ld of its matte surface
        if (hs & HS_LE) le = sc.lights[(hs >> REC_MAT_SHIFT) & 0xffu].Lemit;
        ld = rec.ld + (size_t)slot * ROW;
    } else {
        ld = rec.ld + (size_t)slot * ROW;
        if (hs >> 31) {
            const float4 q = rec.hit_q[slot];
            mat = &sc.materials[(hs >> REC_MAT_SHIFT) & 0xffu];
            const float Ft = mat->is_mc ? 1.f : 1.f - rho_lookup(mat->rho, mat->n_rho, q.w);
            kss = kInvPiF * Ft;
            mo = reinterpret_cast<const float *>(rec.mo4 + (size_t)slot * kGroups);
            if (mat->has_alb_tex) {
                const float4 a = rec.hit_alb[slot];
                arg[0] = a.x;
                arg[1] = a.y;
                arg[2] = a.z;
                alb = true;
            }
        }
    }
    float X = 0.f, Y = 0.f, Z = 0.f;
    bool nan = false;
    for (int c = 0; c < NB; ++c) {
        float L = 0.f;
        if (le) L += le[c];
        if (mo) {
            const float ab = alb ? tex_albedo_pow(arg, c, 1.f - mat->mix) : mat->alb_1mmix[c];
            float t = (kss * mo[mat->band_pos[c]]) * ab;
            t = t < 0.f ? 0.f : t;  // Spectrum::Clamp(0, INFINITY)
            L += t;
        }
        if (ld) L += ld[c];
        nan = nan || (L != L);
        X += kCieX[c] * L;
        Y += kCieY[c] * L;
        Z += kCieZ[c] * L;
        if (SPEC) rec.ld[(size_t)slot * ROW + c] = L;  // (band c of the row is read above)
    }
    const float scale = (float)(700 - 400) / (float)(MPSS_CIE_Y_INTEGRAL * NB);
    const float y = Y * (float)(700 - 400) / (float)(MPSS_CIE_Y_INTEGRAL * NB);
    X *= scale;
    Y *= scale;
    Z *= scale;
    if (nan || y < -1e-5f || __builtin_isinf(y)) X = Y = Z = 0.f;
    rec.xyz[slot] = make_float4(X, Y, Z, 0.f);
    if (SPEC && (nan || y < -1e-5f || __builtin_isinf(y)))
        for (int c = 0; c < NB; ++c) rec.ld[(size_t)slot * ROW + c] = 0.f;
}
template __global__ void assemble_kernel<false>(RenderScene sc, SampleRecs rec, int max_hits);
template __global__ void assemble_kernel<true>(RenderScene sc, SampleRecs rec, int max_hits);

// Camera rays that escaped with infinite lights in the scene (SamplerRenderer::Li,
// samplerrenderer.cpp:144-151): L = 0 + sum over lights of Le(ray), area lights adding 0; then
// the sample filter and ToXYZ as in assemble_kernel. A separate launch keeps assemble_kernel's
// registers (and occupancy) independent of the 30-band sky sum.
template <bool SPEC>
__global__ __launch_bounds__(256) void sky_kernel(RenderScene sc, SampleRecs rec, int max_hits) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int nhits = *rec.hit_count;
    if (slot >= nhits || slot >= max_hits) return;
    const uint32_t hs = rec.hit_s[slot];
    if (!((hs & HS_LIGHT) && !(hs & HS_LSURF))) return;
    const float4 hb = rec.hit_b[slot];
    float Ls[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) Ls[c] = 0.f;
    for (int l = 0; l < sc.nlights; ++l) {
        const RenderLight &Lt = sc.lights[l];
        if (!Lt.kind) continue;
        float s, t, rgb[3];
        inf_coords(Lt, V3{hb.x, hb.y, hb.z}, s, t);
        inf_lookup(Lt, s, t, rgb);
#pragma unroll
        for (int c = 0; c < NB; ++c) Ls[c] += illum_band(rgb, c);
    }
    float X = 0.f, Y = 0.f, Z = 0.f;
    bool nan = false;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const float L = Ls[c];
        nan = nan || (L != L);
        X += kCieX[c] * L;
        Y += kCieY[c] * L;
        Z += kCieZ[c] * L;
    }
    const float scale = (float)(700 - 400) / (float)(MPSS_CIE_Y_INTEGRAL * NB);
    const float y = Y * (float)(700 - 400) / (float)(MPSS_CIE_Y_INTEGRAL * NB);
    X *= scale;
    Y *= scale;
    Z *= scale;
    if (nan || y < -1e-5f || __builtin_isinf(y)) X = Y = Z = 0.f;
    rec.xyz[slot] = make_float4(X, Y, Z, 0.f);
    if (SPEC) {  // an escaped ray has an Ld row of its own like every slot: nothing else uses it
        const bool rej = nan || y < -1e-5f || __builtin_isinf(y);
        float4 *row = reinterpret_cast<float4 *>(rec.ld + (size_t)slot * ROW);
#pragma unroll
        for (int k = 0; k < 7; ++k)
            row[k] = rej ? make_float4(0.f, 0.f, 0.f, 0.f)
                         : make_float4(Ls[4 * k], Ls[4 * k + 1], Ls[4 * k + 2], Ls[4 * k + 3]);
        row[7] = rej ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(Ls[28], Ls[29], 0.f, 0.f);
    }
}
template __global__ void sky_kernel<false>(RenderScene sc, SampleRecs rec, int max_hits);
template __global__ void sky_kernel<true>(RenderScene sc, SampleRecs rec, int max_hits);

__global__ __launch_bounds__(256) void film_kernel(RenderScene sc, PieceList pl, SampleRecs rec) {
    const int k = piece_of(pl, (int)blockIdx.x);
    const TileBatch &tb = pl.tb[k];
    rec.flags += pl.off[k];
    rec.slot += pl.off[k];
    rec.spill += pl.off[k] / tb.spp;
    float *__restrict__ out = pl.out[k];
    const int out_stride_px = pl.out_stride[k];
    const int i = ((int)blockIdx.x - pl.block0[k]) * blockDim.x + threadIdx.x;
    const int tw = tb.x1 - tb.x0, th = tb.y1 - tb.y0;
    if (i >= tw * th) return;
    const int px = tb.x0 + i % tw, py = tb.y0 + i / tw;
    float X = 0.f, Y = 0.f, Z = 0.f, W = 0.f;
    // own samples (always inside this pixel's filter support), then the 8 neighbours' samples
    // in row-major order whose float image position rounds onto the shared edge
    // (ImageFilm::AddSample with the 0.5-wide box filter, image.cpp:77-137). Samples that hit
    // nothing add exactly 0 to X, Y, Z (never -0), so only their weight is accumulated.
    for (int q = 0; q < 9; ++q) {
        const int dx = q == 0 ? 0 : ((q - 1 + (q > 4)) % 3) - 1;
        const int dy = q == 0 ? 0 : ((q - 1 + (q > 4)) / 3) - 1;
        const int qx = px + dx, qy = py + dy;
        if (qx < tb.ex0 || qy < tb.ey0 || qx >= tb.ex0 + tb.ew || qy >= tb.ey0 + tb.eh) continue;
        const int64_t li = (int64_t)(qy - tb.ey0) * tb.ew + (qx - tb.ex0);
        // bits the neighbour's samples need to reach this pixel
        const uint32_t need = (dx < 0 ? REC_XHI : dx > 0 ? REC_XLO : 0u) | (dy < 0 ? REC_YHI : dy > 0 ? REC_YLO : 0u);
        if (q == 0) {
            const int32_t *sl = rec.slot + li * tb.spp;
            if ((tb.spp & 7) == 0) {
                // 8 slots as two 16-byte loads: a lane's run of slots is contiguous, and the
                // vector-memory path pays per cache line an instruction touches, so one wide load
                // per line instead of four narrow ones (same slots, same order)
                const int4 *sl4 = reinterpret_cast<const int4 *>(sl);
                for (int s0 = 0; s0 < tb.spp; s0 += 8) {
                    const int4 a4 = sl4[s0 >> 2], b4 = sl4[(s0 >> 2) + 1];
                    const int32_t v[8] = {a4.x, a4.y, a4.z, a4.w, b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (v[k] >= 0) {
                            const float4 x = rec.xyz[v[k]];
                            X += 1.f * x.x;
                            Y += 1.f * x.y;
                            Z += 1.f * x.z;
                        }
                        W += 1.f;
                    }
                }
                continue;
            }
            for (int s0 = 0; s0 < tb.spp; s0 += 8) {
                int32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = s0 + k < tb.spp ? sl[s0 + k] : -2;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (v[k] == -2) break;
                    if (v[k] >= 0) {
                        const float4 x = rec.xyz[v[k]];
                        X += 1.f * x.x;
                        Y += 1.f * x.y;
                        Z += 1.f * x.z;
                    }
                    W += 1.f;
                }
            }
            continue;
        }
        if ((rec.spill[li] & need) != need) continue;
        for (int s = 0; s < tb.spp; ++s) {
            const int64_t sid = li * tb.spp + s;
            if ((rec.flags[sid] & need) != need) continue;
            const int32_t v = rec.slot[sid];
            if (v >= 0) {
                const float4 x = rec.xyz[v];
                X += 1.f * x.x;
                Y += 1.f * x.y;
                Z += 1.f * x.z;
            }
            W += 1.f;
        }
    }
    float *o = out + ((size_t)(py - tb.y0) * out_stride_px + (px - tb.x0)) * 4;
    o[0] = X;
    o[1] = Y;
    o[2] = Z;
    o[3] = W;
}

// ImageFilm::AddSample (film/image.cpp:77-137) under any other filter, as a gather: no float atomics,
// so a pixel's sums have one order -- the pixels of [py - ry, py + ry] x [px - rx, px + rx] row-major,
// a pixel's samples in index order.
// A workgroup owns a kFilmTile x kFilmTile block of the tile (a lane per pixel) and walks the block plus
// its halo once: the workgroup stages the halo's camera samples in LDS -- image position minus 0.5
// (recomputed from the hash: two words less to store and read back per sample than a float2 buffer
// written by the camera pass) and XYZ, zeros for a sample without radiance, whose weight alone counts:
// w * 0 added to a sum leaves its bits alone -- kFilmStage samples at a time, whole halo rows while
// they fit (at 4 spp and a radius of 2 the whole 20 x 20 halo is one stage), parts of a row beyond.
// Staging reads consecutive slots with consecutive lanes (a halo row's samples are contiguous), then
// one 16-byte XYZ load per sample with radiance. Each lane then runs over its own window of the stage:
// every staged sample is read by up to (2 rx + 1)(2 ry + 1) lanes, from LDS.
// A lane's pixel lies in the frame, so AddSample's clamped range [Ceil(d - w), Floor(d + w)] holds px
// exactly when d - w <= px <= d + w in float.
__global__ __launch_bounds__(256) void film_filter_kernel(RenderScene sc, PieceList pl, SampleRecs rec, FilmFilter f) {
    __shared__ float s_tab[kFilterTableSize * kFilterTableSize];
    __shared__ float s_dx[kFilmStage], s_dy[kFilmStage], s_x[kFilmStage], s_y[kFilmStage], s_z[kFilmStage];
    const int tid = (int)threadIdx.x;
    const int k = piece_of(pl, (int)blockIdx.x);
    const TileBatch &tb = pl.tb[k];
    rec.slot += pl.off[k];
    const int spp = tb.spp;
    const int nbx = (tb.x1 - tb.x0 + kFilmTile - 1) / kFilmTile;
    const int b = (int)blockIdx.x - pl.block0[k];
    const int bx0 = tb.x0 + (b % nbx) * kFilmTile, by0 = tb.y0 + (b / nbx) * kFilmTile;
    const int bx1 = min(bx0 + kFilmTile, tb.x1), by1 = min(by0 + kFilmTile, tb.y1);
    // the block's halo, inside the piece's pixels
    const int hx0 = max(bx0 - f.g.rx, tb.ex0), hx1 = min(bx1 + f.g.rx, tb.ex0 + tb.ew);
    const int hy0 = max(by0 - f.g.ry, tb.ey0), hy1 = min(by1 + f.g.ry, tb.ey0 + tb.eh);
    const int px = bx0 + (tid % kFilmTile), py = by0 + (tid / kFilmTile);
    const bool own = px < bx1 && py < by1;
    const float fpx = (float)px, fpy = (float)py;
    s_tab[tid] = f.table[tid];
    // this lane's window: halo rows [wy0, wy1), and samples [jlo, jhi) of a halo row
    const int row_n = (hx1 - hx0) * spp;
    const int wy0 = max(py - f.g.ry, hy0), wy1 = min(py + f.g.ry + 1, hy1);
    const int jlo = (max(px - f.g.rx, hx0) - hx0) * spp, jhi = (min(px + f.g.rx + 1, hx1) - hx0) * spp;
    const int rows = row_n <= kFilmStage ? kFilmStage / row_n : 1;
    const int cols = row_n <= kFilmStage ? row_n : kFilmStage;
    float X = 0.f, Y = 0.f, Z = 0.f, W = 0.f;
    for (int r0 = hy0; r0 < hy1; r0 += rows) {
        const int r1 = min(r0 + rows, hy1);
        for (int j0 = 0; j0 < row_n; j0 += cols) {
            const int j1 = min(j0 + cols, row_n), nj = j1 - j0;
            __syncthreads();  // the table is written; the stage before this one is read
            const int n = (r1 - r0) * nj;  // <= kFilmStage
            for (int i = tid; i < n; i += 256) {
                const int qy = r0 + i / nj, j = j0 + i % nj;
                const int qx = hx0 + j / spp, s = j % spp;
                float sx, sy;
                image_sample_keyed(tb.seed, filter_pixel_key(f.g, sc.xres, sc.yres, qx, qy), qx, qy, s, sx, sy);
                const int32_t v = rec.slot[((int64_t)(qy - tb.ey0) * tb.ew + (qx - tb.ex0)) * spp + s];
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v >= 0) x = rec.xyz[v];
                s_dx[i] = sx - 0.5f;
                s_dy[i] = sy - 0.5f;
                s_x[i] = x.x;
                s_y[i] = x.y;
                s_z[i] = x.z;
            }
            __syncthreads();
            if (!own) continue;
            const int ja = max(j0, jlo), jb = min(j1, jhi);
            for (int qy = max(r0, wy0); qy < min(r1, wy1); ++qy) {
                const int base = (qy - r0) * nj - j0;
                for (int j = ja; j < jb; ++j) {
                    const int i = base + j;
                    const float dx = s_dx[i], dy = s_dy[i];
                    if (!(dx - f.g.wx <= fpx && dx + f.g.wx >= fpx && dy - f.g.wy <= fpy && dy + f.g.wy >= fpy)) continue;
                    const float w = s_tab[filter_index(py, dy, f.g.inv_wy) * kFilterTableSize +
                                          filter_index(px, dx, f.g.inv_wx)];
                    X += w * s_x[i];
                    Y += w * s_y[i];
                    Z += w * s_z[i];
                    W += w;
                }
            }
        }
    }
    if (!own) return;
    float *o = pl.out[k] + ((size_t)(py - tb.y0) * pl.out_stride[k] + (px - tb.x0)) * 4;
    o[0] = X;
    o[1] = Y;
    o[2] = Z;
    o[3] = W;
}

}  // namespace mpss
