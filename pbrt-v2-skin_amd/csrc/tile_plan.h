// tile_plan.h -- the host planner of render_tiles: rectangles -> row pieces -> batches (-> replay
// windows) -> launch groups. Integer arithmetic on plain data (no HIP, no device pointers), so a CPU
// program can link tile_plan.cpp alone (tests/tile_plan_host).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mpss {

// A tile [x0,x1) x [y0,y1) extended by one pixel on every side that exists (origin ex0, ey0;
// ew x eh pixels): a sample whose float image coordinate rounds onto a pixel edge also lands
// in the neighbouring pixel (film_kernel). Under a non-default pixel filter the extension is the
// filter's halo inside the film's sample extent (PlanHalo below), and ex0, ey0 may be negative.
// A kernel argument (render.h PieceList).
struct TileBatch {
    int x0, x1, y0, y1, ex0, ey0, ew, eh, spp;
    uint32_t seed;
    int64_t nsamples;  // ew * eh * spp
};

// pieces of one batch per launch of primary_kernel / film_kernel (render.h PieceList)
constexpr int kMaxPieces = 16;

// A row piece of rectangle `rect`: its rows' samples, and where its pixels start in the
// rectangle's output (floats: (y0 of the piece - y0 of the rectangle) * width * 4).
struct PlanPiece {
    TileBatch tb;
    int rect;
    size_t out_off;
};

// Pieces [first, end) rendered together: `total` camera samples, bounding box [bx0, bx1) x [by0, by1)
// of the extended pieces. Replay sampler: the generated window [wx0, wx1) x [wy0, wy1) in force for
// the batch, and whether it is generated before this batch (new_window) or carried from an earlier one.
struct PlanBatch {
    size_t first, end;
    int64_t total;
    int bx0, bx1, by0, by1;
    bool new_window;
    int wx0, wx1, wy0, wy1;
};

struct TilePlan {
    std::vector<PlanPiece> pieces;
    std::vector<PlanBatch> batches;
};

// Up to kMaxPieces consecutive pieces of a batch, from piece `first`, in one launch of `blocks` workgroups:
// piece j owns blocks [block0[j], block0[j + 1]); its camera samples start at record off[j] of the
// batch (counted over the whole batch, not the group); out_stride[j]: its rectangle's width.
struct LaunchGroup {
    size_t first;
    int n, blocks;
    int block0[kMaxPieces + 1];
    int out_stride[kMaxPieces];
    int64_t off[kMaxPieces];
};

// r = {x0, x1, y0, y1}: a non-empty rectangle inside the W x H frame
bool tile_rect_ok(const int32_t *r, int W, int H);

// Cuts the n rectangles (rects[4 i ..] = x0, x1, y0, y1) into row pieces and packs the pieces into
// batches of <= max_batch camera samples (a batch's first piece is always taken). replay: the
// rectangles in (y0, x0) order (stable), each batch's box within window_limit floats at spp *
// replay_k floats per pixel, and the windows: a new one where a batch's box leaves the window in
// force, extended over the following pieces up to the first that would not fit.
TilePlan plan_tiles(int W, int H, int spp, uint32_t seed, int n, const int32_t *rects, int64_t max_batch,
                    bool replay, int replay_k, int64_t window_limit);

// How far a piece reaches beyond its tile: (rx, ry) pixels (a filter's halo radius, pixel_filter.h),
// clipped to [xs, xe) x [ys, ye). The default filter: one pixel, clipped to the frame -- what the
// overload above plans with. Another filter: its halo, clipped to the film's sample extent, so pieces at
// the image edge hold out-of-frame pixels (ex0 / ey0 < 0, ex0 + ew > W).
struct PlanHalo {
    int rx, ry, xs, xe, ys, ye;
};
TilePlan plan_tiles(int W, int H, int spp, uint32_t seed, int n, const int32_t *rects, int64_t max_batch,
                    bool replay, int replay_k, int64_t window_limit, const PlanHalo &halo);

// The launches of batch b; blocks per piece: ceil(items / 256) of its samples (primary_kernel) or, for
// film, its tile pixels (film_kernel); film_tile > 0: one block per film_tile x film_tile pixels of the tile
// (film_filter_kernel).
std::vector<LaunchGroup> launch_groups(const TilePlan &plan, const PlanBatch &b, bool film, int film_tile = 0);

}  // namespace mpss
