// film_spectral.hip -- the films of a spectral call (mpss_render_tile_spectral): ImageFilm::AddSample
// (film/image.cpp:77-137) over the samples' 30-band L instead of their XYZ. assemble_kernel<true> and
// sky_kernel<true> (film.hip) leave a sample's L in its hit's Ld row, 32 floats = one 128-byte line.
//   film_spectral_kernel         the 0.5-wide box filter: film_kernel's walk
//   film_filter_spectral_kernel  any other filter: film_filter_kernel's staging and walk
// Both give a pixel eight adjacent lanes, lane g the bands 4 g .. 4 g + 3: a sample's row is one line read as
// float4 by neighbouring lanes, a pixel's output row one 128-byte store. Every lane of a pixel walks the same
// samples in the same order with the same weights as the XYZ film's lane does, so a band's sum has that
// film's order and the weight sum (every lane carries it; lane 7 stores it in slot 30, 0 in slot 31) its bits.
#include "film_spectral.h"

#include "geom.h"

namespace mpss {

// the rows' bands of lane g, w times, onto a
__device__ __forceinline__ void add_row(float4 &a, float w, const float *ld, int32_t v, int g) {
    const float4 x = reinterpret_cast<const float4 *>(ld + (size_t)v * ROW)[g];
    a.x += w * x.x;
    a.y += w * x.y;
    a.z += w * x.z;
    a.w += w * x.w;
}

// the pixel's output row: lane 7 holds bands 28 and 29, then the weight sum and 0
__device__ __forceinline__ void store_row(float *out, size_t pixel, int g, float4 a, float W) {
    if (g == kSpecLanes - 1) {
        a.z = W;
        a.w = 0.f;
    }
    reinterpret_cast<float4 *>(out + pixel * ROW)[g] = a;  // (ROW = MPSS_SPECTRAL_ROW: render_host.hip)
}

__global__ __launch_bounds__(256) void film_spectral_kernel(RenderScene sc, PieceList pl, SampleRecs rec) {
    const int k = piece_of(pl, (int)blockIdx.x);
    const TileBatch &tb = pl.tb[k];
    rec.flags += pl.off[k];
    rec.slot += pl.off[k];
    rec.spill += pl.off[k] / tb.spp;
    const int t = ((int)blockIdx.x - pl.block0[k]) * (int)blockDim.x + (int)threadIdx.x;
    const int i = t / kSpecLanes, g = t % kSpecLanes;
    const int tw = tb.x1 - tb.x0, th = tb.y1 - tb.y0;
    if (i >= tw * th) return;  // (the eight lanes of a pixel leave together)
    const int px = tb.x0 + i % tw, py = tb.y0 + i / tw;
    const int lane = (int)(threadIdx.x & 63u), lane0 = lane - g;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    float W = 0.f;
    // film_kernel's order: own samples, then the 8 neighbours' row-major. The pixel's lanes load eight
    // consecutive samples' slots (and flags) with one instruction and hand them round: every branch below
    // depends on the pixel alone, so its eight lanes are always active together.
    for (int q = 0; q < 9; ++q) {
        const int dx = q == 0 ? 0 : ((q - 1 + (q > 4)) % 3) - 1;
        const int dy = q == 0 ? 0 : ((q - 1 + (q > 4)) / 3) - 1;
        const int qx = px + dx, qy = py + dy;
        if (qx < tb.ex0 || qy < tb.ey0 || qx >= tb.ex0 + tb.ew || qy >= tb.ey0 + tb.eh) continue;
        const int64_t li = (int64_t)(qy - tb.ey0) * tb.ew + (qx - tb.ex0);
        const uint32_t need = (dx < 0 ? REC_XHI : dx > 0 ? REC_XLO : 0u) | (dy < 0 ? REC_YHI : dy > 0 ? REC_YLO : 0u);
        if (q != 0 && (rec.spill[li] & need) != need) continue;
        for (int s0 = 0; s0 < tb.spp; s0 += kSpecLanes) {
            const int64_t sid = li * tb.spp + s0 + g;
            const bool have = s0 + g < tb.spp;
            const int32_t mine = have ? rec.slot[sid] : -1;
            // own samples always count; a neighbour's when its position rounds onto the shared edge
            const int take = have && (q == 0 || (rec.flags[sid] & need) == need) ? 1 : 0;
            for (int j = 0; j < kSpecLanes; ++j) {
                const int32_t v = __shfl(mine, lane0 + j);
                if (!__shfl(take, lane0 + j)) continue;
                if (v >= 0) add_row(a, 1.f, rec.ld, v, g);
                W += 1.f;
            }
        }
    }
    store_row(pl.out[k], (size_t)(py - tb.y0) * pl.out_stride[k] + (px - tb.x0), g, a, W);
}

// film_filter_kernel with a kSpecTileX x kSpecTileY block of pixels per workgroup, eight lanes a pixel. The
// stage holds a sample's image offsets and its hit slot (-1: no radiance, its weight alone counts) in place of
// its XYZ: 12 bytes a sample, 24 KB a stage and 1 KB of table, six workgroups a CU by LDS. The bands come from
// the hit's row in global memory, one line per (sample, pixel) pair read by the pixel's eight lanes at once.
__global__ __launch_bounds__(256) void film_filter_spectral_kernel(RenderScene sc, PieceList pl, SampleRecs rec,
                                                                   FilmFilter f) {
    __shared__ float s_tab[kFilterTableSize * kFilterTableSize];
    __shared__ float s_dx[kFilmStage], s_dy[kFilmStage];
    __shared__ int32_t s_slot[kFilmStage];
    const int tid = (int)threadIdx.x;
    const int k = piece_of(pl, (int)blockIdx.x);
    const TileBatch &tb = pl.tb[k];
    rec.slot += pl.off[k];
    const int spp = tb.spp;
    const int nbx = (tb.x1 - tb.x0 + kSpecTileX - 1) / kSpecTileX;
    const int b = (int)blockIdx.x - pl.block0[k];
    const int bx0 = tb.x0 + (b % nbx) * kSpecTileX, by0 = tb.y0 + (b / nbx) * kSpecTileY;
    const int bx1 = min(bx0 + kSpecTileX, tb.x1), by1 = min(by0 + kSpecTileY, tb.y1);
    // the block's halo, inside the piece's pixels
    const int hx0 = max(bx0 - f.g.rx, tb.ex0), hx1 = min(bx1 + f.g.rx, tb.ex0 + tb.ew);
    const int hy0 = max(by0 - f.g.ry, tb.ey0), hy1 = min(by1 + f.g.ry, tb.ey0 + tb.eh);
    const int p = tid / kSpecLanes, g = tid % kSpecLanes;
    const int px = bx0 + (p % kSpecTileX), py = by0 + (p / kSpecTileX);
    const bool own = px < bx1 && py < by1;
    const float fpx = (float)px, fpy = (float)py;
    s_tab[tid] = f.table[tid];
    // this pixel's window: halo rows [wy0, wy1), and samples [jlo, jhi) of a halo row
    const int row_n = (hx1 - hx0) * spp;
    const int wy0 = max(py - f.g.ry, hy0), wy1 = min(py + f.g.ry + 1, hy1);
    const int jlo = (max(px - f.g.rx, hx0) - hx0) * spp, jhi = (min(px + f.g.rx + 1, hx1) - hx0) * spp;
    const int rows = row_n <= kFilmStage ? kFilmStage / row_n : 1;
    const int cols = row_n <= kFilmStage ? row_n : kFilmStage;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    float W = 0.f;
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
                s_dx[i] = sx - 0.5f;
                s_dy[i] = sy - 0.5f;
                s_slot[i] = rec.slot[((int64_t)(qy - tb.ey0) * tb.ew + (qx - tb.ex0)) * spp + s];
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
                    const int32_t v = s_slot[i];
                    if (v >= 0) add_row(a, w, rec.ld, v, g);
                    W += w;
                }
            }
        }
    }
    if (!own) return;
    store_row(pl.out[k], (size_t)(py - tb.y0) * pl.out_stride[k] + (px - tb.x0), g, a, W);
}

}  // namespace mpss
