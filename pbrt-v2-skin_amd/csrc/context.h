// context.h -- per-integrator state behind the C ABI (one mpss_ctx per
// MultipoleSubsurfaceIntegrator instance; reference integrators/multipolesubsurface.h:36-80).
#pragma once
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/mpss.h"
#include "common.h"
#include "dipole.h"
#include "material.h"
#include "mo_kernel.h"
#include "octree.h"
#include "pixel_filter.h"
#include "replay.h"
#include "scene.h"
#include "texture_build.h"
#include "tile_plan.h"

namespace mpss {

struct RenderScene;

struct Material {
    ProfileTables profile;
    RhoTable rho;
    float albedo[NB];
    float Kr[NB];              // Microfacet reflectance (layeredskin "Kr")
    float Kt[NB];              // MicrofacetTransmission transmittance (layeredskin "Kt")
    float roughness = 0.4f, ior = 1.4f;
    bool double_ref_sslf = false;
    bool is_monte_carlo = false;
    // "genprofile" false (layeredskin.cpp:70,120-122): no MultipoleBSSRDF data -- no Mo() term on its
    // surfaces, its irradiance points lit as points without a BSSRDF; the tables are a zero placeholder
    bool no_bssrdf = false;
    DeviceProfile dev_profile;
    DevBuf<float> dev_rho;  // [n_rho]
    int albedo_tex = -1, bump_tex = -1;  // ImageTexture ids ("texture albedo" / "texture bumpmap")
    int kr_tex = -1, kt_tex = -1;        // ... ("texture Kr" / "texture Kt"): evaluated per camera hit
    // rgbprofile (ComputeRGBMultipoleProfile): Rd = FromRGB of three tables, Mo() in the
    // reference-order gather; dev_rgb [3][L] (rows 0..2 of profile.table), rgb_rcp their rcp
    bool rgb = false;
    DevBuf<float> dev_rgb, dev_rgb_rcp;
    float rgb_rcp[3] = {0.f, 0.f, 0.f};
    // a DiffusionReflectance functor instead of a profile (mpss_add_dipole_material): Mo only
    bool dipole = false;
    DipoleRd dip{};
    DevBuf<float> dev_dipole;  // [4][NB] zpos, zneg, sigma_tr, k
};

// ImageTexture<RGBSpectrum, Spectrum> / ImageTexture<float, float> (textures/imagemap.{h,cpp})
// with its UVMapping2D: the converted texels' MIPMap, on the host and (after upload) the device.
struct ImageTexture {
    HostPyramid py;
    int trilinear = 0;
    float max_aniso = 8.f, su = 1.f, sv = 1.f, du = 0.f, dv = 0.f;
    TexView host;  // over py.data
    DevBuf<float> dev;
    TexView device_view(const float *lut) const {
        TexView v = host;
        v.data = dev.ptr;
        v.lut = lut;
        return v;
    }
};
// ImageTexture::GetTexture's conversion + MIPMap (imagemap.cpp:55-84): texels through convertIn,
// or the one-valued map when the image could not be read (width == 0)
std::unique_ptr<ImageTexture> build_imagemap(const mpss_imagemap &m);

// Device workspace of one render_tiles (or mo_batch) call. Calls on different streams may run
// at once (pbrt calls Li from every worker thread), so each call takes a workspace of its own
// from the context's pool; `done` (recorded on the call's stream) orders a later user of the
// same workspace after the kernels of the previous one.
// Per-sample buffers (flags, slot, and the hit records primary_kernel writes: ha, hb, hs) are sized
// for the batch's camera samples; everything after the hit compaction (Mo() queries and results,
// direct-light terms, XYZ) for the batch's actual hit count, which render_tiles reads back once per
// batch. Every buffer records its own size (DevBuf::n) and only grows, through reserve().
struct RenderWorkspace {
    DevBuf<uint32_t> flags, hs, spill;
    DevBuf<int32_t> slot;
    DevBuf<int> count, work, perm;  // perm: the sharded gather's sorted query ids
    DevBuf<float4> q, mo, ha, hb, xyz, alb, frame, st, kr, kt;
    DevBuf<unsigned char> terms;
    DevBuf<float> ld;
    // reference-sampler replay: the batch's window table and the render tasks' stream cursors
    // (render.h ReplayCursors; valid for rp_key = {scene generation, spp, tasks})
    DevBuf<float> rp_table;
    DevBuf<uint32_t> rp_mt;
    DevBuf<int> rp_pix, rp_mti;
    uint64_t rp_key[3] = {~0ull, 0, 0};
    hipEvent_t done = nullptr;
    int device = 0;
    bool pending = false;
    // buf holds at least `count` elements. A buffer is reallocated only once the kernels of the
    // workspace's previous user are done: the host waits for them when, and only when, buf grows.
    template <class T>
    void reserve(DevBuf<T> &buf, size_t count) {
        if (buf.n >= count) return;
        if (pending) MPSS_HIP(hipEventSynchronize(done));
        buf.alloc(count);
    }
    ~RenderWorkspace();
};

class Context {
public:
    explicit Context(const mpss_config &cfg);
    ~Context();
    uint32_t add_layeredskin(const mpss_layeredskin &m);
    // rebuilds material `id` in place (mpss_update_layeredskin): what add_layeredskin builds for m, under
    // the same id, texture bindings and meshes; the Preprocess-derived irradiance goes stale
    void update_layeredskin(uint32_t id, const mpss_layeredskin &m);
    uint32_t set_material_tables(const float *rd, uint32_t len, const float *rcp, const float *rho, uint32_t n_rho,
                                 const float *albedo, bool is_mc);
    // the single-dipole Rd of the dipolesubsurface integrator (dipole.h); usable with mo_batch
    uint32_t add_dipole_material(const float *sigma_a, const float *sigmap_s, float eta);
    // copies under mu_ (a material may be rebuilt in place by update_layeredskin: no reference to one
    // leaves the lock); sizes are always written, the buffers are nullable
    void material_tables(uint32_t id, float *rd, uint32_t *len, float *rcp, float *rho, uint32_t *n_rho,
                         float *total) const;
    void gather_info(uint32_t id, int *common_grid, float *rel_err, float *l1_err) const;
    // the common grid the context built for material `id` and LDS layout near_field (mpss_get_common_grid;
    // outputs as mpss_host_common_grid)
    void common_grid(uint32_t id, int near_field, float *rows, uint32_t *n_rows, int32_t *bands, float *rg,
                     float *u0lim, float *u1lim, float *u1start, uint32_t *row0, uint32_t *ubase, float *rel_err,
                     float *l1_err, float *ua, float *hinv, int *ok) const;
    // monotonic counts since creation: scene uploads, point-set builds, material table builds, octree builds
    void build_counts(uint64_t counts[4]) const;
    void set_irradiance_points(int n, const float *p, const float *nrm, const float *E, const float *area);
    const DeviceOctree &octree() const;
    void export_octree(void *nodes, float *node_et, float *pt_hdr, float *pt_e, int32_t *pt_index);
    uint32_t add_imagemap(const mpss_imagemap &m);
    void set_material_textures(uint32_t material, int albedo, int bump);
    void set_material_spec_textures(uint32_t material, int kr, int kt);
    std::vector<const TexView *> host_bump_views() const;
    float max_error() const { return max_error_; }
    GatherOpts gather_opts() const {
        GatherOpts o;
        o.near_field = cfg_.mo_near_field;
        o.steal = cfg_.mo_work_stealing != 0;
        o.count_noprune = cfg_.count_traversal == 2;
        o.common_grid = cfg_.mo_common_grid != 0;
        return o;
    }
    const mpss_config &config() const { return cfg_; }

    // scene (scene_upload.hip), Preprocess (preprocess_host.hip), tiled rendering (render_host.hip)
    void add_mesh(uint32_t nv, const float *P, const float *N, const float *S, const float *uv, uint32_t nt,
                  const int32_t *idx, const float *o2w, const float *w2o, bool reverse, uint32_t material);
    void add_sphere_light(const float *c, float r, const float *Lemit, int nsamples);
    // texels: W x H RGB (nullable: no "mapname", the 1x1 map L.ToRGBSpectrum())
    void add_infinite_light(const float *L, int nsamples, const float *l2w, const float *w2l, int W = 0, int H = 0,
                            const float *texels = nullptr);
    void set_camera(const float *r2c, const float *c2w, int xres, int yres);
    void set_surface_points(uint32_t n, const SurfacePoint *pts);
    void preprocess(uint32_t seed);
    void tessellate_on_gpu();  // Preprocess point set, GPU build (preprocess_host.hip)
    // FindPoissonPointDistribution (usepoissonpointfinder): fills points_ (preprocess_host.hip)
    void find_poisson_points(uint32_t seed);
    // spec (mpss_render_tiles_spectral): per rectangle, its rows of MPSS_SPECTRAL_ROW floats per pixel; outs,
    // or any outs[i], may then be null (no XYZW film for that rectangle)
    void render_tiles(int spp, uint32_t seed, int n, const int32_t *rects, float *const *outs, hipStream_t stream,
                      float *const *spec = nullptr);
    // the replay sampler's table (mpss_replay_samples); out may be null to query sizes
    void replay_samples(int spp, float *out, uint64_t *n_floats, int *k);
    void check_replay_lds(int spp, const char *who) const;  // replay_check_lds over the scene's lights
    // SubsurfaceOctreeNode::Mo over q device-resident points with material `mid`'s profile
    // (mpss_mo_batch); stream-ordered, safe for concurrent callers on their own streams
    void mo_batch(uint32_t mid, int q, const float *p_dev, float *out_dev, int32_t *counters_dev, hipStream_t stream,
                  unsigned long long *counts_dev = nullptr);
    // the sharded gather's instrumented pass over a batch: stats[kGroups][kStatStride] (mo_kernel.h), synchronous
    void mo_batch_paths(uint32_t mid, int q, const float *p_dev, float *out_dev, uint64_t *stats);
    // Cost probe for tile dealing: one camera ray through every pixel centre; per rect, the rays
    // that hit a BSSRDF surface (sss) and any mesh surface (surf). Synchronous.
    void tile_costs(int n, const int32_t *rects, int64_t *sss, int64_t *surf);
    // copies under mu_ (the point set is cached across Preprocess calls and dropped by mutators)
    std::vector<SurfacePoint> surface_points() const {
        std::lock_guard<std::mutex> g(mu_);
        return points_;
    }
    std::vector<float> irradiance() const {
        std::lock_guard<std::mutex> g(mu_);
        return irradiance_;
    }
    // for calls that use the context's device but none of its state (mpss_profile_fit, mpss_sog_fit):
    // makes the device current and serialises the call against the context's other calls
    std::unique_lock<std::mutex> lock_device() const {
        activate();
        return std::unique_lock<std::mutex>(mu_);
    }
    bool has_octree() const { return have_octree_; }
    mpss_render_stats render_stats();
    void reset_render_stats();
    // which builder later material builds use for the common grids' per-knot scan (mpss_set_grid_builder)
    void set_grid_builder(bool on_host) {
        std::lock_guard<std::mutex> g(mu_);
        grid_on_host_ = on_host;
    }
    // the film's reconstruction filter of later renders (mpss_set_pixel_filter); checked by the caller
    void set_pixel_filter(const PixelFilter &f) {
        std::lock_guard<std::mutex> g(mu_);
        filter_ = f;
    }
    void set_instrumentation(bool timing, int counting) {
        std::lock_guard<std::mutex> g(mu_);
        cfg_.kernel_timing = timing;
        cfg_.count_traversal = counting;
    }

private:
    void activate() const;
    void upload_scene();
    // its steps, in order (scene_upload.hip; mu_ held); upload_materials is the last
    void upload_bvh();
    void upload_camera_bins();
    void upload_meshes();
    void upload_lights();
    void upload_textures();
    // the materials' device records alone (d_materials_): all a material update changes of the scene
    void upload_materials();
    // the device scene is current: upload_scene when the scene changed, upload_materials when only a
    // material was rebuilt (mu_ held)
    void sync_scene_locked() {
        if (scene_dirty_)
            upload_scene();
        else if (materials_dirty_)
            upload_materials();
    }
    // anything tessellation or the Poisson point finder reads has changed (meshes, lights, camera, texture
    // bindings, the material list): points the context built itself are found again by the next
    // Preprocess; a caller's points (set_surface_points) stay, only their device copy is dropped (mu_ held)
    void mark_scene_dirty_locked() {
        scene_dirty_ = true;
        invalidate_points_locked();
    }
    void invalidate_points_locked() {
        if (points_src_ == PointsSrc::Built) points_src_ = PointsSrc::None;
        pc_.valid = false;
    }
    std::unique_ptr<Material> build_layeredskin(const mpss_layeredskin &m);
    // mpss_render_tile(s) / mpss_tile_costs after a material update and before the next Preprocess
    void require_fresh_irradiance(const char *who) const;
    RenderScene render_scene() const;
    // the steps of preprocess, in order (preprocess_host.hip; mu_ held): the point set exists, its point
    // cache pc_ is valid, the irradiance at its n points is in irradiance_ (and dE, when a kernel ran)
    void preprocess_points(uint32_t seed);
    void preprocess_point_cache(int n);
    void preprocess_irradiance(int n, uint32_t seed, float *dE);
    int first_bssrdf_material() const;
    // reference-sampler replay (mpss_config.sampler): floats per camera sample in the window tables,
    // and the scene generation the workspaces' task cursors belong to (upload_scene bumps it)
    int replay_k_ = kReplayImage;
    uint64_t scene_gen_ = 0;
    // the window [x0, x1) x [y0, y1) of the sample extent at spp into ws->rp_table (the cursors in ws
    // reset when the scene, spp or task count changed); on `stream`
    // all_values: every sample's light-sample values (the whole table, replay_samples), not only those
    // of samples whose camera ray hits (all a render reads)
    void replay_window(RenderWorkspace *ws, const RenderScene &sc, int spp, int x0, int x1, int y0, int y1,
                       hipStream_t stream, bool all_values = false);
    // The steps of one render_tiles batch, in order (render_host.hip; mu_ not held). A TileCall is the
    // call's constants: stream, workspace, sampling and instrumentation settings, BSSRDF materials.
    struct TileCall;
    void batch_begin(const TileCall &c, int64_t total);
    void batch_window(TileCall &c, RenderScene &sc, const PlanBatch &b);
    void launch_pieces(const TileCall &c, const RenderScene &sc, const TilePlan &plan, const PlanBatch &b, bool film);
    int batch_primary(TileCall &c, const RenderScene &sc, const TilePlan &plan, const PlanBatch &b);
    void batch_reserve_hits(const TileCall &c, const RenderScene &sc, int64_t nh);
    void batch_direct(TileCall &c, const RenderScene &sc, int64_t nh);
    void batch_mo(TileCall &c, int64_t nh);
    void batch_film(TileCall &c, const RenderScene &sc, const TilePlan &plan, const PlanBatch &b, int64_t nh);
    void launch_films_spectral(const TileCall &c, const RenderScene &sc, const TilePlan &plan, const PlanBatch &b);
    SceneData scene_;
    bool scene_dirty_ = true, materials_dirty_ = false;
    // where points_ came from: the caller (set_surface_points / pointsfile) or a Preprocess of this
    // context (tessellation or the Poisson finder, with points_seed_)
    enum class PointsSrc { None, User, Built };
    PointsSrc points_src_ = PointsSrc::None;
    uint32_t points_seed_ = 0;
    std::vector<SurfacePoint> points_;
    // Preprocess's arrays of points_ (position, normal, ray epsilon, material, uv; area on the host):
    // they depend on the point set alone, so they are kept across Preprocess calls (pigment sweeps)
    struct PointCache {
        bool valid = false;
        std::vector<float> p, nr, area;
        DevBuf<float> dp, dn, de, duv;
        DevBuf<uint32_t> dm;
    } pc_;
    // irradiance_ and the octree came from a Preprocess (not from set_irradiance_points), and a
    // material was rebuilt since: renders are refused until the next Preprocess
    bool preprocessed_ = false, irradiance_stale_ = false;
    bool grid_on_host_ = false;  // (the GPU scan is the default: BASELINE.md section 3, "Pigment sweep")
    uint64_t n_scene_uploads_ = 0, n_point_builds_ = 0, n_material_builds_ = 0, n_octree_builds_ = 0;
    std::vector<float> irradiance_;
    DevBuf<BvhNode> d_bvh_;
    DevBuf<BvhNode> d_bvh_thread_;  // threaded copy (interior offset = end of subtree), any-hit walks
    DevBuf<TriRec> d_tris_;
    // reference sampler: the camera rays' candidate triangles per pixel (scene.h CameraBins)
    DevBuf<uint32_t> d_bin_off_;
    DevBuf<int32_t> d_bin_tri_, d_bin_all_;
    int bin_w_ = 0, bin_nall_ = 0;
    DevBuf<int32_t> d_tri_mesh_, d_tri_local_;
    std::vector<std::unique_ptr<DevBuf<float>>> d_mesh_bufs_;
    DevBuf<struct RenderMesh> d_meshes_;
    DevBuf<struct RenderLight> d_lights_;
    std::vector<std::unique_ptr<DevBuf<float>>> d_envmaps_;  // per infinite light (envmap.h layout)
    DevBuf<float> d_zero_map_;                                // stand-in map of area lights
    DevBuf<struct RenderMaterial> d_materials_;
    std::vector<std::unique_ptr<ImageTexture>> textures_;
    DevBuf<float> d_lut_;  // EWA weight table
    // workspace pool (render_tiles / mo_batch); guarded by mu_
    std::vector<std::unique_ptr<RenderWorkspace>> ws_free_;
    RenderWorkspace *acquire_ws();
    void release_ws(RenderWorkspace *ws, hipStream_t stream);
    hipError_t release_ws_nothrow(RenderWorkspace *ws, hipStream_t stream) noexcept;  // for unwinding paths
    // One in-flight call (inflight_ already counted under mu_): on every way out of the call, exceptions
    // included, its workspace returns to the pool and the count drops (so quiesce_locked never waits
    // for a call that has failed). mu_ must not be held when the guard dies.
    struct InflightGuard {
        Context *c;
        RenderWorkspace *ws;
        hipStream_t stream;
        void release() {  // the normal path: hands the workspace back, throwing on a HIP error
            RenderWorkspace *w = ws;
            ws = nullptr;
            if (w) c->release_ws(w, stream);
        }
        ~InflightGuard() {
            if (ws) (void)c->release_ws_nothrow(ws, stream);
            c->end_inflight();
        }
    };
    // every BSSRDF material's band layout exists on the device octree (mu_ held)
    void ensure_layouts();
    // p, nrm, E, area: host arrays; dp / dn / dE (nullable): the same on the device, when the caller
    // has them there already (Preprocess)
    void build_octree_locked(int n, const float *p, const float *nrm, const float *E, const float *area,
                             const float *dp = nullptr, const float *dn = nullptr, const float *dE = nullptr);
    // serializes everything that changes the context (scene, materials, octree, stats) and the
    // workspace pool; launches happen outside it
    mutable std::mutex mu_;
    // render_tiles / mo_batch calls between taking their device pointers (under mu_) and queueing
    // their last kernel; a call that replaces what they read (octree and band layouts, scene
    // buffers, replay table) first waits for none to be in flight, then for the queued kernels
    // (quiesce_locked). Guarded by mu_.
    int inflight_ = 0;
    std::condition_variable_any idle_;
    void quiesce_locked();
    void end_inflight();
    // kernel timing (cfg_.kernel_timing) and traversal counting (cfg_.count_traversal): render_stats.cpp
    struct Timed {
        hipEvent_t a, b;
        int kind;
    };
    std::vector<Timed> timed_;  // guarded by mu_
    void time_begin(bool on, hipStream_t s, hipEvent_t &a);
    void time_end(bool on, hipStream_t s, hipEvent_t a, int kind, std::vector<Timed> &out);
    mpss_render_stats stats_{};
    DevBuf<unsigned long long> d_counts_;  // [kStatStride * kGroups] traversal counts (mo_kernel.h)
    mpss_config cfg_;
    PixelFilter filter_;  // guarded by mu_; a render works on its own copy (TileCall)
    float max_error_, min_dist_;
    std::vector<std::unique_ptr<Material>> materials_;

    DeviceOctree dev_octree_;
    bool have_octree_ = false;
};

}  // namespace mpss
