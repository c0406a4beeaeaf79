// render_host.hip -- host driver of tiled rendering: the reference sampler's replay windows, and
// render_tiles as a plan (tile_plan.h) and its per-batch steps over the primary.hip, shade.hip, film.hip
// and Mo() gather kernels; the tile-cost probe. (The scene: scene_upload.hip; Preprocess:
// preprocess_host.hip; timing and counters: render_stats.cpp.)
#include <algorithm>
#include <cstring>

#include "context.h"
#include "film_filter.h"
#include "film_spectral.h"
#include "render.h"

namespace mpss {

// The reference sampler's values over [x0, x1) x [y0, y1) of the sample extent at `spp`
// (replay_gen.hip) into ws->rp_table, continuing the workspace's task streams.
void Context::replay_window(RenderWorkspace *ws, const RenderScene &sc, int spp, int x0, int x1, int y0, int y1,
                            hipStream_t stream, bool all_values) {
    const int W = sc.xres, H = sc.yres;
    const int T = replay_render_tasks(W, H, std::max(1, cfg_.replay_cores));
    const uint64_t key[3] = {scene_gen_, (uint64_t)spp, (uint64_t)T};
    if (ws->pending) MPSS_HIP(hipStreamWaitEvent(stream, ws->done, 0));  // the workspace's previous user
    if (ws->rp_key[0] != key[0] || ws->rp_key[1] != key[1] || ws->rp_key[2] != key[2]) {
        ws->reserve(ws->rp_mt, (size_t)624 * T);
        ws->reserve(ws->rp_pix, (size_t)T);
        ws->reserve(ws->rp_mti, (size_t)T);
        MPSS_HIP(hipMemsetAsync(ws->rp_pix.ptr, 0xff, sizeof(int) * (size_t)T, stream));  // -1: not seeded
        for (int k = 0; k < 3; ++k) ws->rp_key[k] = key[k];
    }
    ws->reserve(ws->rp_table, (size_t)(x1 - x0) * (y1 - y0) * spp * replay_k_);
    ReplayWindow w{};
    replay_window_tasks(W, H, T, x0, x1, y0, y1, w);
    w.spp = spp;
    w.K = replay_k_;
    w.li_draws = (cfg_.max_depth > 0 && !cfg_.show_irradiance_points) ? kReplayLiDraws : 0;
    w.nmax = 1;
    w.nlights = (int)scene_.lights.size();
    w.arr_draws = 0;
    for (const SceneLight &l : scene_.lights) {
        const int n = replay_round_up_pow2(l.nsamples);
        w.nmax = std::max(w.nmax, n);
        w.arr_draws += 3 * (spp * n + spp) + 5;
    }
    w.cur = ReplayCursors{ws->rp_mt.ptr, ws->rp_pix.ptr, ws->rp_mti.ptr};
    w.out = ws->rp_table.ptr;
    if (!d_bin_off_.ptr || bin_w_ != W + 1) throw Error(MPSS_ERR_INTERNAL, "replay: no camera-ray bins for this camera");
    w.bin_off = d_bin_off_.ptr;
    w.bin_tri = d_bin_tri_.ptr;
    w.bin_all = d_bin_all_.ptr;
    w.bin_w = bin_w_;
    w.bin_nall = bin_nall_;
    w.all_values = all_values ? 1 : 0;
    launch_replay_window(sc, w, stream);
}

void Context::check_replay_lds(int spp, const char *who) const {
    std::vector<int> ns;
    for (const SceneLight &l : scene_.lights) ns.push_back(l.nsamples);
    replay_check_lds(spp, ns.data(), (int)ns.size(), who);
}

void Context::replay_samples(int spp, float *out, uint64_t *n_floats, int *k) {
    activate();
    std::unique_lock<std::mutex> lk(mu_);
    if (cfg_.sampler != MPSS_SAMPLER_REFERENCE) throw Error(MPSS_ERR_INVALID, "replay_samples: the context uses the hash sampler");
    sync_scene_locked();
    const int W = scene_.camera.xres, H = scene_.camera.yres;
    if (W <= 0) throw Error(MPSS_ERR_INVALID, "replay_samples: no camera");
    spp = replay_round_up_pow2(spp);
    if (spp > kReplayMaxSpp) throw Error(MPSS_ERR_INVALID, "replay_samples: spp too large for the replay sampler");
    check_replay_lds(spp, "replay_samples");
    const int K = replay_k_;
    *k = K;
    const int64_t npix = (int64_t)(W + 1) * (H + 1);
    *n_floats = (uint64_t)npix * spp * K;
    if (!out) return;
    // the whole sample extent as one window, on a workspace of its own cursors
    RenderWorkspace *ws = acquire_ws();
    ++inflight_;
    RenderScene sc = render_scene();
    lk.unlock();
    InflightGuard guard{this, ws, nullptr};
    replay_window(ws, sc, spp, 0, W + 1, 0, H + 1, nullptr, true);
    std::vector<float> col((size_t)npix * spp * K);
    MPSS_HIP(hipMemcpy(col.data(), ws->rp_table.ptr, sizeof(float) * col.size(), hipMemcpyDeviceToHost));
    ws->rp_key[0] = ~0ull;  // (its cursors now sit at the end of every stream)
    guard.release();
    // column-major window -> the documented layout [((y (W + 1) + x) spp + s) K + k]
    for (int64_t p = 0; p < npix; ++p)
        for (int s2 = 0; s2 < spp; ++s2)
            for (int c = 0; c < K; ++c) out[(p * spp + s2) * K + c] = col[((size_t)c * npix + p) * spp + s2];
}

// One render_tiles call's constants, as its batch steps read them (mu_ not held: what they name of the
// context -- scene buffers, materials, octree -- is only read).
struct Context::TileCall {
    hipStream_t stream;
    RenderWorkspace *ws;
    float *const *outs;  // per rectangle
    // a spectral call (mpss_render_tile(s)_spectral): per rectangle, rows of ROW floats per pixel; outs, or
    // outs[i], may then be null. Null: an XYZ call.
    float *const *spec;
    int spp;
    uint32_t seed;
    int nlights, ns_max;
    bool timing;
    unsigned long long *counts;  // traversal counters (null: not counting)
    // every LayeredSkin material has a MultipoleBSSRDF (GetMultipoleBSSRDF, layeredskin.cpp:180-185):
    // each evaluates Mo() with its own profile (multipolesubsurface.cpp:267-280)
    struct SssMat {
        int id;
        const Material *m;
        const BandLayout *layout;
    };
    std::vector<SssMat> sss;
    float max_error;
    GatherOpts gopts;
    // a non-default pixel filter (pixel_filter.h): the *_filter_kernel instances run, over pieces that
    // reach `ff.g.rx, ry` pixels beyond their tiles
    bool filtered;
    FilmFilter ff;
    std::vector<Timed> timed;
    // (the per-hit pointers are valid after batch_reserve_hits)
    SampleRecs recs() const {
        return SampleRecs{ws->flags.ptr, ws->spill.ptr, ws->slot.ptr, ws->ld.ptr, ws->ha.ptr, ws->hb.ptr, ws->hs.ptr,
                          ws->q.ptr,     ws->count.ptr, ws->mo.ptr,   ws->xyz.ptr, ws->alb.ptr, ws->frame.ptr,
                          ws->kr.ptr,    ws->kt.ptr};
    }
};

// per-sample buffers: the batch's camera samples (primary_kernel may give each a hit slot)
void Context::batch_begin(const TileCall &c, int64_t total) {
    RenderWorkspace *ws = c.ws;
    ws->reserve(ws->flags, (size_t)total);
    ws->reserve(ws->slot, (size_t)total);
    ws->reserve(ws->ha, (size_t)total);
    ws->reserve(ws->hb, (size_t)total);
    ws->reserve(ws->hs, (size_t)total);
    ws->reserve(ws->spill, (size_t)(total / c.spp));
    MPSS_HIP(hipMemsetAsync(ws->count.ptr, 0, sizeof(int), c.stream));
    MPSS_HIP(hipMemsetAsync(ws->spill.ptr, 0, sizeof(uint32_t) * (size_t)(total / c.spp), c.stream));
}

// replay: the reference sampler's values over the batch's window, when the plan starts a new one
void Context::batch_window(TileCall &c, RenderScene &sc, const PlanBatch &b) {
    if (!b.new_window) return;
    hipEvent_t ev{};
    time_begin(c.timing, c.stream, ev);
    replay_window(c.ws, sc, c.spp, b.wx0, b.wx1, b.wy0, b.wy1, c.stream);
    time_end(c.timing, c.stream, ev, 6, c.timed);
    sc.replay = c.ws->rp_table.ptr;
    sc.replay_x0 = b.wx0;
    sc.replay_y0 = b.wy0;
    sc.replay_w = b.wx1 - b.wx0;
    sc.replay_npix = (int64_t)(b.wx1 - b.wx0) * (b.wy1 - b.wy0);
}

// the batch's pieces, kMaxPieces per launch, through primary_kernel or film_kernel
void Context::launch_pieces(const TileCall &c, const RenderScene &sc, const TilePlan &plan, const PlanBatch &b,
                            bool film) {
    for (const LaunchGroup &g : launch_groups(plan, b, film, c.filtered ? kFilmTile : 0)) {
        PieceList pl{};
        pl.n = g.n;
        for (int j = 0; j < g.n; ++j) {
            const PlanPiece &p = plan.pieces[g.first + j];
            pl.block0[j] = g.block0[j];
            pl.tb[j] = p.tb;
            pl.off[j] = g.off[j];
            float *const o = c.outs[p.rect];  // (null: a spectral call's rectangle without an XYZW output)
            pl.out[j] = o ? o + p.out_off : nullptr;
            pl.out_stride[j] = g.out_stride[j];
        }
        pl.block0[g.n] = g.blocks;
        if (film && c.filtered)
            hipLaunchKernelGGL(film_filter_kernel, dim3((unsigned)g.blocks), dim3(256), 0, c.stream, sc, pl, c.recs(),
                               c.ff);
        else if (film)
            hipLaunchKernelGGL(film_kernel, dim3((unsigned)g.blocks), dim3(256), 0, c.stream, sc, pl, c.recs());
        else if (c.filtered)
            hipLaunchKernelGGL(primary_filter_kernel, dim3((unsigned)g.blocks), dim3(256), 0, c.stream, sc, pl, c.recs(),
                               c.ff.g);
        else
            hipLaunchKernelGGL(primary_kernel, dim3((unsigned)g.blocks), dim3(256), 0, c.stream, sc, pl, c.recs());
    }
}

// primary_kernel over the batch; returns the batch's hit count, which sizes everything after the
// compaction: one read-back per batch (the stream only waits for primary_kernel; the GPU idles for the
// round trip alone)
int Context::batch_primary(TileCall &c, const RenderScene &sc, const TilePlan &plan, const PlanBatch &b) {
    hipEvent_t ev{};
    time_begin(c.timing, c.stream, ev);
    launch_pieces(c, sc, plan, b, false);
    time_end(c.timing, c.stream, ev, 1, c.timed);
    int nh_dev = 0;
    MPSS_HIP(hipMemcpyAsync(&nh_dev, c.ws->count.ptr, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    MPSS_HIP(hipStreamSynchronize(c.stream));
    return nh_dev;
}

// per-hit buffers: Mo() queries and results, direct light, XYZ, the gather's query order, texture lookups
void Context::batch_reserve_hits(const TileCall &c, const RenderScene &sc, int64_t nh) {
    RenderWorkspace *ws = c.ws;
    ws->reserve(ws->q, (size_t)nh);
    ws->reserve(ws->xyz, (size_t)nh);
    ws->reserve(ws->mo, (size_t)nh * kGroups);
    ws->reserve(ws->ld, (size_t)nh * ROW);
    ws->reserve(ws->perm, (size_t)((nh + 1023) / 1024 * 1024));
    if (sc.any_tex) {
        ws->reserve(ws->alb, (size_t)nh);
        ws->reserve(ws->frame, (size_t)nh * 2);
    }
    if (sc.any_spec_tex) {
        ws->reserve(ws->kr, (size_t)nh);
        ws->reserve(ws->kt, (size_t)nh);
    }
}

// texture lookups, then UniformSampleAllLights: a lane per (hit, light, light sample), combined per hit
void Context::batch_direct(TileCall &c, const RenderScene &sc, int64_t nh) {
    RenderWorkspace *ws = c.ws;
    const hipStream_t stream = c.stream;
    const int64_t lanes = nh * std::max<int64_t>(1, (int64_t)c.nlights) * c.ns_max;
    if (lanes > (int64_t)INT32_MAX)
        throw Error(MPSS_ERR_INVALID, "render_tile: too many light samples per batch; lower "
                                      "max_batch_samples");
    ws->reserve(ws->terms, (size_t)lanes * 64);
    DirectTerms *terms = reinterpret_cast<DirectTerms *>(ws->terms.ptr);
    float4 *inf_st = nullptr;
    if (sc.n_infinite > 0) {
        ws->reserve(ws->st, (size_t)lanes);
        inf_st = ws->st.ptr;
    }
    const SampleRecs rec = c.recs();
    const dim3 per_hit((unsigned)((nh + 255) / 256));
    hipEvent_t ev{};
    // a scene with Kr / Kt textures (any_spec_tex) runs the *_spec_kernel instances, every other scene the
    // kernels it always ran
    if (sc.any_spec_tex) {
        time_begin(c.timing, stream, ev);
        if (c.filtered)
            hipLaunchKernelGGL(shade_tex_filter_spec_kernel, per_hit, dim3(256), 0, stream, sc, rec, c.spp, c.seed,
                               (int)nh, c.ff.g);
        else
            hipLaunchKernelGGL(shade_tex_spec_kernel, per_hit, dim3(256), 0, stream, sc, rec, c.spp, c.seed, (int)nh);
        time_end(c.timing, stream, ev, 5, c.timed);
    } else if (sc.any_tex) {
        time_begin(c.timing, stream, ev);
        if (c.filtered)
            hipLaunchKernelGGL(shade_tex_filter_kernel, per_hit, dim3(256), 0, stream, sc, rec, c.spp, c.seed, (int)nh,
                               c.ff.g);
        else
            hipLaunchKernelGGL(shade_tex_kernel, per_hit, dim3(256), 0, stream, sc, rec, c.spp, c.seed, (int)nh);
        time_end(c.timing, stream, ev, 5, c.timed);
    }
    time_begin(c.timing, stream, ev);
    if (c.nlights > 0 && sc.any_spec_tex) {
        hipLaunchKernelGGL(shade_direct_spec_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, sc,
                           rec, c.spp, c.seed, (int)nh, c.ns_max, terms, inf_st);
        if (sc.n_infinite > 0)
            hipLaunchKernelGGL(direct_combine_spec_kernel<true>, per_hit, dim3(256), 0, stream, sc, rec, (int)nh,
                               c.ns_max, (const DirectTerms *)terms, (const float4 *)inf_st);
        else
            hipLaunchKernelGGL(direct_combine_spec_kernel<false>, per_hit, dim3(256), 0, stream, sc, rec, (int)nh,
                               c.ns_max, (const DirectTerms *)terms, (const float4 *)nullptr);
    } else if (c.nlights > 0) {
        hipLaunchKernelGGL(shade_direct_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, sc, rec,
                           c.spp, c.seed, (int)nh, c.ns_max, terms, inf_st);
        if (sc.n_infinite > 0)
            hipLaunchKernelGGL(direct_combine_kernel<true>, per_hit, dim3(256), 0, stream, sc, rec, (int)nh, c.ns_max,
                               (const DirectTerms *)terms, (const float4 *)inf_st);
        else
            hipLaunchKernelGGL(direct_combine_kernel<false>, per_hit, dim3(256), 0, stream, sc, rec, (int)nh, c.ns_max,
                               (const DirectTerms *)terms, (const float4 *)nullptr);
    } else {
        hipLaunchKernelGGL(shade_nolight_kernel, per_hit, dim3(256), 0, stream, sc, rec, (int)nh);
    }
    time_end(c.timing, stream, ev, 4, c.timed);
}

// ONE sharded Mo() gather per BSSRDF material over the batch's hits
void Context::batch_mo(TileCall &c, int64_t nh) {
    if (c.sss.empty()) return;
    RenderWorkspace *ws = c.ws;
    hipEvent_t ev{};
    time_begin(c.timing, c.stream, ev);
    for (const TileCall::SssMat &s : c.sss)  // (an rgbprofile material: FromRGB of its R, G, B lookups)
        launch_mo_band(dev_octree_, *s.layout, s.m->dev_profile, c.max_error, (int)nh, ws->q.ptr, ws->count.ptr,
                       ws->mo.ptr, c.sss.size() > 1 ? ws->hs.ptr : nullptr, s.id, c.counts, ws->work.ptr, ws->perm.ptr,
                       c.gopts, c.stream);
    time_end(c.timing, c.stream, ev, 2, c.timed);
}

// A spectral call's films over the batch's pieces: the band film into every piece's rows of the cube, and
// the XYZ film (the kernels of an XYZ call) into the pieces of rectangles that have an XYZW output. The launch
// groups are launch_pieces'; the band films' workgroups hold 256 / kSpecLanes pixels.
void Context::launch_films_spectral(const TileCall &c, const RenderScene &sc, const TilePlan &plan,
                                    const PlanBatch &b) {
    static_assert(ROW == MPSS_SPECTRAL_ROW, "a cube row is a hit's Ld row");
    for (const LaunchGroup &g : launch_groups(plan, b, true, c.filtered ? kFilmTile : 0)) {
        PieceList xyz{}, sp{};
        xyz.n = sp.n = g.n;
        int nx = 0, ns = 0;
        for (int j = 0; j < g.n; ++j) {
            const PlanPiece &p = plan.pieces[g.first + j];
            const int tw = p.tb.x1 - p.tb.x0, th = p.tb.y1 - p.tb.y0;
            float *const o = c.outs[p.rect];
            xyz.block0[j] = nx;
            sp.block0[j] = ns;
            xyz.tb[j] = sp.tb[j] = p.tb;
            xyz.off[j] = sp.off[j] = g.off[j];
            xyz.out_stride[j] = sp.out_stride[j] = g.out_stride[j];
            xyz.out[j] = o ? o + p.out_off : nullptr;  // (no XYZW output: no blocks)
            sp.out[j] = c.spec[p.rect] + p.out_off * (ROW / 4);
            if (o) nx += g.block0[j + 1] - g.block0[j];
            ns += c.filtered ? ((tw + kSpecTileX - 1) / kSpecTileX) * ((th + kSpecTileY - 1) / kSpecTileY)
                             : (int)(((int64_t)tw * th * kSpecLanes + 255) / 256);
        }
        xyz.block0[g.n] = nx;
        sp.block0[g.n] = ns;
        if (c.filtered) {
            hipLaunchKernelGGL(film_filter_spectral_kernel, dim3((unsigned)ns), dim3(256), 0, c.stream, sc, sp,
                               c.recs(), c.ff);
            if (nx > 0)
                hipLaunchKernelGGL(film_filter_kernel, dim3((unsigned)nx), dim3(256), 0, c.stream, sc, xyz, c.recs(),
                                   c.ff);
        } else {
            hipLaunchKernelGGL(film_spectral_kernel, dim3((unsigned)ns), dim3(256), 0, c.stream, sc, sp, c.recs());
            if (nx > 0) hipLaunchKernelGGL(film_kernel, dim3((unsigned)nx), dim3(256), 0, c.stream, sc, xyz, c.recs());
        }
    }
}

// Li assembly per hit, the sky behind the misses, then the filtered film per piece
void Context::batch_film(TileCall &c, const RenderScene &sc, const TilePlan &plan, const PlanBatch &b, int64_t nh) {
    const SampleRecs rec = c.recs();
    const dim3 per_hit((unsigned)((nh + 255) / 256));
    hipEvent_t ev{};
    time_begin(c.timing, c.stream, ev);
    if (c.spec) {
        hipLaunchKernelGGL(assemble_kernel<true>, per_hit, dim3(256), 0, c.stream, sc, rec, (int)nh);
        if (sc.n_infinite > 0) hipLaunchKernelGGL(sky_kernel<true>, per_hit, dim3(256), 0, c.stream, sc, rec, (int)nh);
        launch_films_spectral(c, sc, plan, b);
        time_end(c.timing, c.stream, ev, 3, c.timed);
        MPSS_HIP(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL(assemble_kernel<false>, per_hit, dim3(256), 0, c.stream, sc, rec, (int)nh);
    if (sc.n_infinite > 0) hipLaunchKernelGGL(sky_kernel<false>, per_hit, dim3(256), 0, c.stream, sc, rec, (int)nh);
    launch_pieces(c, sc, plan, b, true);
    time_end(c.timing, c.stream, ev, 3, c.timed);
    MPSS_HIP(hipGetLastError());
}

// SamplerRenderer::Render restricted to pixel rectangles. plan_tiles (tile_plan.h) cuts each rectangle
// into row pieces (a piece = the rows plus the border of samples that the pixel filter carries in: one
// pixel for the default box, the filter's halo otherwise) and packs the pieces into batches of <= max_batch_samples camera samples. Per batch:
// camera kernel over the pieces (all pieces append their surface hits to one compacted list) -> direct
// lighting per hit -> ONE sharded Mo() gather per BSSRDF material over the batch's hits -> film kernel
// over the pieces. Calls on different streams may overlap: each takes its own workspace (RenderWorkspace),
// and the scene, materials and octree are only read after the context lock is released.
void Context::render_tiles(int spp, uint32_t seed, int n, const int32_t *rects, float *const *outs,
                           hipStream_t stream, float *const *spec) {
    activate();
    std::unique_lock<std::mutex> lk(mu_);
    require_fresh_irradiance("render_tile");
    sync_scene_locked();
    const int W = scene_.camera.xres, H = scene_.camera.yres;
    if (W <= 0) throw Error(MPSS_ERR_INVALID, "render_tile: no camera");
    if (spp < 1 || spp > 65535) throw Error(MPSS_ERR_INVALID, "render_tile: spp must be in [1, 65535]");
    const bool replay = cfg_.sampler == MPSS_SAMPLER_REFERENCE;
    if (replay) {
        spp = replay_round_up_pow2(spp);  // LDSampler rounds pixelsamples up (lowdiscrepancy.cpp:45-49)
        if (spp > kReplayMaxSpp)
            throw Error(MPSS_ERR_INVALID, "render_tile: spp must be at most 4096 for the replay sampler");
        check_replay_lds(spp, "render_tile");
        // the replay's windows and pbrt's task split are laid out over the default filter's sample extent
        if (!filter_.is_default())
            throw Error(MPSS_ERR_INVALID, "render_tile: the reference sampler renders only with the default pixel "
                                          "filter (box 0.5 / 0.5); set that filter or use the hash sampler");
    }
    std::vector<float *> no_outs;  // a spectral call without XYZW outputs: a null one per rectangle
    if (spec && !outs) {
        no_outs.assign((size_t)std::max(n, 1), nullptr);
        outs = no_outs.data();
    }
    for (int i = 0; i < n; ++i) {
        if (!tile_rect_ok(rects + 4 * i, W, H)) throw Error(MPSS_ERR_INVALID, "render_tile: bad rectangle");
        if (spec ? !spec[i] : !outs[i]) throw Error(MPSS_ERR_INVALID, "render_tile: null output");
    }
    TileCall c{};
    c.stream = stream;
    c.outs = outs;
    c.spec = spec;
    c.spp = spp;
    c.seed = seed;
    c.filtered = !filter_.is_default();
    if (c.filtered) c.ff = film_filter(filter_, W, H);
    const PlanHalo halo = filter_plan_halo(filter_, W, H);
    if (have_octree_)
        for (size_t i = 0; i < materials_.size(); ++i)
            if (!materials_[i]->dipole && !materials_[i]->no_bssrdf)
                c.sss.push_back(TileCall::SssMat{(int)i, materials_[i].get(),
                                                 &dev_octree_.ensure_layout(materials_[i]->dev_profile.groups)});
    RenderScene sc = render_scene();
    sc.have_octree = c.sss.empty() ? 0 : 1;
    if (replay) {  // (the window and its table: per batch, batch_window)
        sc.replay_k = replay_k_;
        sc.replay_spp = spp;
    }
    const bool counting = cfg_.count_traversal != 0;
    c.timing = cfg_.kernel_timing != 0;
    if (counting && !d_counts_.ptr) {
        d_counts_.alloc(kStatStride * kGroups);
        MPSS_HIP(hipMemset(d_counts_.ptr, 0, kStatStride * kGroups * sizeof(unsigned long long)));
    }
    c.counts = counting ? d_counts_.ptr : nullptr;
    const int64_t max_batch = std::max<int64_t>(cfg_.max_batch_samples, 1 << 10);
    c.nlights = (int)scene_.lights.size();
    c.ns_max = 1;
    for (const SceneLight &l : scene_.lights) c.ns_max = std::max(c.ns_max, replay_round_up_pow2(l.nsamples));
    c.max_error = max_error_;
    c.gopts = gather_opts();
    const int replay_k = replay_k_;
    RenderWorkspace *ws = c.ws = acquire_ws();
    ++inflight_;  // until this call's kernels are queued (see quiesce_locked)
    lk.unlock();
    InflightGuard guard{this, ws, stream};  // every way out: workspace back to the pool, inflight_ down

    const TilePlan plan = plan_tiles(W, H, spp, seed, n, rects, max_batch, replay, replay_k, kReplayWindowFloats, halo);
    int64_t n_samples = 0, n_sss = 0;
    if (ws->pending) MPSS_HIP(hipStreamWaitEvent(stream, ws->done, 0));
    for (const PlanBatch &b : plan.batches) {
        batch_begin(c, b.total);
        batch_window(c, sc, b);
        const int nh_dev = batch_primary(c, sc, plan, b);
        const int64_t nh = std::max<int64_t>(1, nh_dev);
        batch_reserve_hits(c, sc, nh);
        batch_direct(c, sc, nh);
        batch_mo(c, nh);
        batch_film(c, sc, plan, b, nh);
        n_samples += b.total;
        if (counting) n_sss += nh_dev;
    }
    guard.release();
    std::lock_guard<std::mutex> g(mu_);  // (released before the guard's end_inflight takes mu_)
    timed_.insert(timed_.end(), c.timed.begin(), c.timed.end());
    stats_.samples += n_samples;
    stats_.sss_samples += n_sss;
}

// Tile-cost probe (mpss_tile_costs): classes per pixel centre, summed per rectangle on the host.
void Context::tile_costs(int n, const int32_t *rects, int64_t *sss, int64_t *surf) {
    activate();
    std::lock_guard<std::mutex> g(mu_);
    require_fresh_irradiance("tile_costs");
    sync_scene_locked();
    const int W = scene_.camera.xres, H = scene_.camera.yres;
    if (W <= 0) throw Error(MPSS_ERR_INVALID, "tile_costs: no camera");
    RenderScene sc = render_scene();
    sc.have_octree = have_octree_ ? 1 : 0;
    DevBuf<uint8_t> cls;
    cls.alloc((size_t)W * H);
    hipLaunchKernelGGL(probe_kernel, dim3((unsigned)(((int64_t)W * H + 255) / 256)), dim3(256), 0, 0, sc, 0, W, 0, H,
                       cls.ptr);
    MPSS_HIP(hipGetLastError());
    std::vector<uint8_t> h((size_t)W * H);
    MPSS_HIP(hipMemcpy(h.data(), cls.ptr, h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const int32_t *r = rects + 4 * i;
        if (!tile_rect_ok(r, W, H)) throw Error(MPSS_ERR_INVALID, "tile_costs: bad rectangle");
        int64_t a = 0, b = 0;
        for (int y = r[2]; y < r[3]; ++y)
            for (int x = r[0]; x < r[1]; ++x) {
                const uint8_t c = h[(size_t)y * W + x];
                a += c == 2;
                b += c >= 1;
            }
        sss[i] = a;
        surf[i] = b;
    }
}

}  // namespace mpss
