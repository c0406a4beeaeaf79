// preprocess_host.hip -- host driver of Preprocess: the surface-point set (the caller's, tessellated on the
// GPU or the host, or the Poisson finder's), the irradiance kernel over it and the octree build
// (preprocess_kernels.hip, tess_kernel.h kernels).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"
#include "poisson_accept.h"
#include "render.h"
#include "spectral.h"

namespace mpss {

void Context::set_surface_points(uint32_t n, const SurfacePoint *pts) {
    std::lock_guard<std::mutex> g(mu_);
    points_.assign(pts, pts + n);
    points_src_ = n > 0 ? PointsSrc::User : PointsSrc::None;
    pc_.valid = false;
}

// TessellateSurfacePointsRenderer's point set on the GPU (tess_kernel): per mesh a counting pass,
// a prefix sum of the per-triangle counts on the host (one int64 per triangle), then the emitting
// pass; the points come back to points_ (mpss_get_surface_points / the pointsfile read them there).
void Context::tessellate_on_gpu() {
    const RenderScene sc = render_scene();
    std::vector<int64_t> base(scene_.meshes.size() + 1, 0);
    for (size_t m = 0; m < scene_.meshes.size(); ++m)
        base[m + 1] = base[m] + (int64_t)(scene_.meshes[m].idx.size() / 3);
    const int64_t ntri = base.back();
    points_.clear();
    if (ntri == 0) return;
    DevBuf<int64_t> cnt, off;
    cnt.alloc((size_t)ntri);
    off.alloc((size_t)ntri);
    for (size_t m = 0; m < scene_.meshes.size(); ++m) {
        const int nt = (int)(base[m + 1] - base[m]);
        if (nt > 0)
            hipLaunchKernelGGL((tess_kernel<false, false>), dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, 0, sc,
                               (int)m, nt, base[m], min_dist_, cnt.ptr, (const int64_t *)nullptr,
                               (SurfacePoint *)nullptr);
    }
    MPSS_HIP(hipGetLastError());
    std::vector<int64_t> h((size_t)ntri);
    MPSS_HIP(hipMemcpy(h.data(), cnt.ptr, sizeof(int64_t) * (size_t)ntri, hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (int64_t i = 0; i < ntri; ++i) {
        const int64_t c = h[(size_t)i];
        h[(size_t)i] = total;
        total += c;
    }
    if (total > ((int64_t)1 << 30)) throw Error(MPSS_ERR_INVALID, "tessellation: more than 2^30 surface points");
    if (total == 0) return;
    MPSS_HIP(hipMemcpy(off.ptr, h.data(), sizeof(int64_t) * (size_t)ntri, hipMemcpyHostToDevice));
    DevBuf<SurfacePoint> pts;
    pts.alloc((size_t)total);
    for (size_t m = 0; m < scene_.meshes.size(); ++m) {
        const int nt = (int)(base[m + 1] - base[m]);
        if (nt > 0) {
            void (*emit)(RenderScene, int, int, int64_t, float, int64_t *, const int64_t *, SurfacePoint *) =
                cfg_.incenter ? tess_kernel<true, true> : tess_kernel<true, false>;
            hipLaunchKernelGGL(emit, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, 0, sc, (int)m, nt, base[m],
                               min_dist_, cnt.ptr, (const int64_t *)off.ptr, pts.ptr);
        }
    }
    MPSS_HIP(hipGetLastError());
    points_.resize((size_t)total);
    MPSS_HIP(hipMemcpy(points_.data(), pts.ptr, sizeof(SurfacePoint) * (size_t)total, hipMemcpyDeviceToHost));
}

// MultipoleSubsurfaceIntegrator::Preprocess (multipolesubsurface.cpp:170-238)
void Context::preprocess(uint32_t seed) {
    activate();
    std::lock_guard<std::mutex> g(mu_);
    quiesce_locked();  // no render of the previous octree may still be in flight or running
    sync_scene_locked();
    // (on every regular way out: the irradiance and octree, or their absence, are this Preprocess's)
    auto fresh = [&] {
        preprocessed_ = true;
        irradiance_stale_ = false;
    };
    if (scene_.lights.empty()) {  // "if (scene->lights.size() == 0) return;" -> no octree, no SSS
        have_octree_ = false;
        irradiance_.clear();
        fresh();
        return;
    }
    preprocess_points(seed);
    const int n = (int)points_.size();
    if (n == 0) {
        // the reference goes on with an empty point set: its octree holds nothing, so Mo() is 0
        // and the frame has direct lighting only (surfacepoints.cpp:277-281, Preprocess :192-236)
        fprintf(stderr, "mpss: Warning: no surface points with BSSRDFs were found; rendering without "
                        "subsurface scattering\n");
        have_octree_ = false;
        irradiance_.clear();
        fresh();
        return;
    }
    preprocess_point_cache(n);
    DevBuf<float> dE;
    dE.alloc((size_t)n * NB);
    preprocess_irradiance(n, seed, dE.ptr);
    const bool e_on_device = !cfg_.show_irradiance_points;  // dE holds the irradiance kernel's output
    build_octree_locked(n, pc_.p.data(), pc_.nr.data(), irradiance_.data(), pc_.area.data(), pc_.dp.ptr, pc_.dn.ptr,
                        e_on_device ? dE.ptr : nullptr);
    fresh();
}

// The point set exists. It depends on the meshes, min_sample_distance, incenter, the bump maps bound to
// the meshes' materials (tessellation), and on the scene bounds with the area lights, the camera
// position and the seed (Poisson finder) -- not on a material's tables: points built by an earlier
// Preprocess are kept until one of those changes (mark_scene_dirty_locked), so a Preprocess after a
// material update runs the irradiance kernel and the octree build only.
void Context::preprocess_points(uint32_t seed) {
    if (points_src_ == PointsSrc::None ||
        (points_src_ == PointsSrc::Built && cfg_.use_poisson_point_finder && seed != points_seed_)) {
        pc_.valid = false;
        points_src_ = PointsSrc::None;
        if (cfg_.use_poisson_point_finder)
            find_poisson_points(seed);
        else if (cfg_.tessellate_on_host)
            tessellate_surface_points(scene_, min_dist_, cfg_.incenter != 0, points_, 0, host_bump_views().data());
        else
            tessellate_on_gpu();
        points_src_ = PointsSrc::Built;
        points_seed_ = seed;
        ++n_point_builds_;
    }
}

// The point cache is valid: the n points' arrays, host and device, until the point set changes
void Context::preprocess_point_cache(int n) {
    if (pc_.valid) return;
    std::vector<float> eps(n), uv(2 * (size_t)n);
    std::vector<uint32_t> mat(n);
    pc_.p.resize(3 * (size_t)n);
    pc_.nr.resize(3 * (size_t)n);
    pc_.area.resize(n);
    for (int i = 0; i < n; ++i) {
        uv[2 * (size_t)i] = points_[i].u;
        uv[2 * (size_t)i + 1] = points_[i].v;
        for (int k = 0; k < 3; ++k) {
            pc_.p[3 * (size_t)i + k] = points_[i].p[k];
            pc_.nr[3 * (size_t)i + k] = points_[i].n[k];
        }
        eps[i] = points_[i].ray_eps;
        mat[i] = points_[i].material;
        pc_.area[i] = points_[i].area;
    }
    pc_.duv.upload(uv.data(), uv.size());
    pc_.dp.upload(pc_.p.data(), pc_.p.size());
    pc_.dn.upload(pc_.nr.data(), pc_.nr.size());
    pc_.de.upload(eps.data(), eps.size());
    pc_.dm.upload(mat.data(), mat.size());
    pc_.valid = true;
}

// Irradiance at the n cached points into irradiance_ (and dE [n * NB] on the device, when a kernel
// computed it): IrradianceTask (multipolesubsurface.cpp:185-236)
void Context::preprocess_irradiance(int n, uint32_t seed, float *dE) {
    const RenderScene sc = render_scene();
    if (cfg_.show_irradiance_points) {  // IrradianceTask: red points instead of irradiance
        const float red[3] = {1.f, 0.f, 0.f};
        float s[NB];
        spectrum_from_rgb(red, false, s);
        irradiance_.resize((size_t)n * NB);
        for (int i = 0; i < n; ++i) memcpy(&irradiance_[(size_t)i * NB], s, sizeof(s));
    } else {
        RenderScene sci = sc;
        DevBuf<uint32_t> scr, mt;
        if (cfg_.sampler == MPSS_SAMPLER_REFERENCE && !scene_.lights.empty()) {  // IrradianceTask streams
            const int T = replay_irradiance_tasks(n, std::max(1, cfg_.replay_cores));
            scr.alloc((size_t)n * scene_.lights.size() * 2);
            mt.alloc((size_t)624 * T);
            hipLaunchKernelGGL(replay_irradiance_kernel, dim3((T + 63) / 64), dim3(64), 0, 0, n,
                               (int)scene_.lights.size(), T, mt.ptr, scr.ptr);
            MPSS_HIP(hipGetLastError());
            sci.irr_scr = scr.ptr;
        }
        hipEvent_t ev{};
        time_begin(cfg_.kernel_timing != 0, 0, ev);
        hipLaunchKernelGGL(irradiance_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, sci, pc_.dp.ptr, pc_.dn.ptr,
                           pc_.de.ptr, pc_.dm.ptr, pc_.duv.ptr, n, seed, dE);
        MPSS_HIP(hipGetLastError());
        time_end(cfg_.kernel_timing != 0, 0, ev, 0, timed_);
        irradiance_.resize((size_t)n * NB);
        MPSS_HIP(hipMemcpy(irradiance_.data(), dE, sizeof(float) * irradiance_.size(), hipMemcpyDeviceToHost));
    }
}

namespace {
// scene->WorldBound().BoundingSphere(): the bound of every triangle and every area-light sphere
SphereView world_bounding_sphere(const SceneData &scene) {
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = scene.bvh[0].bmin[k];
        hi[k] = scene.bvh[0].bmax[k];
    }
    for (const SceneLight &l : scene.lights) {
        if (l.kind != 0) continue;
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], l.center[k] + -l.radius);
            hi[k] = std::max(hi[k], l.center[k] + l.radius);
        }
    }
    const V3 c = V3{.5f * lo[0] + .5f * hi[0], .5f * lo[1] + .5f * hi[1], .5f * lo[2] + .5f * hi[2]};
    const bool inside = c.x >= lo[0] && c.x <= hi[0] && c.y >= lo[1] && c.y <= hi[1] && c.z >= lo[2] && c.z <= hi[2];
    const float rad = inside ? length(c - V3{hi[0], hi[1], hi[2]}) : 0.f;  // BBox::BoundingSphere
    return full_sphere(c, rad);
}
}  // namespace

// FindPoissonPointDistribution -> SurfacePointsRenderer::Render (renderers/surfacepoints.cpp:115-150)
// with ONE SurfacePointTask (:175-284; the reference runs one per core and its result depends on
// their interleaving): batches of 20000 paths from pCamera are traced on the GPU, 16 batches per
// launch; on the host each batch's candidates are taken in path order and accepted or not by
// PoissonAccept (poisson_accept.h), until maxFails candidates in a row fail.
void Context::find_poisson_points(uint32_t seed) {
    sync_scene_locked();
    activate();
    PoissonWalk w{};
    w.bound = world_bounding_sphere(scene_);
    w.origin = xform_point(scene_.camera.camera_to_world, V3{0.f, 0.f, 0.f});
    w.seed = mix32(seed * 37u + 0x5eed1u);  // RNG rng(37 * taskNum), replay mode
    const int max_fails = cfg_.quick_render ? std::max(10, 2000 / 10) : 2000;
    const float md = min_dist_;
    const float area = kPiF * (md / 2.f) * (md / 2.f);
    constexpr int kBatch = 20000, kBatchesPerLaunch = 16;
    DevBuf<SurfacePoint> dcand;
    DevBuf<int> dcount;
    dcand.alloc((size_t)kBatch * kBatchesPerLaunch * kPoissonCand);
    dcount.alloc((size_t)kBatch * kBatchesPerLaunch);
    std::vector<SurfacePoint> cand((size_t)kBatch * kBatchesPerLaunch * kPoissonCand);
    std::vector<int> cnt((size_t)kBatch * kBatchesPerLaunch);
    PoissonAccept accept(md, max_fails, area);
    points_.clear();
    const RenderScene sc = render_scene();
    PoissonAccept::State state = PoissonAccept::State::GoOn;
    for (uint32_t launch = 0; state == PoissonAccept::State::GoOn; ++launch) {
        w.path0 = launch * (uint32_t)(kBatch * kBatchesPerLaunch);
        w.npaths = kBatch * kBatchesPerLaunch;
        hipLaunchKernelGGL(poisson_walk_kernel, dim3((unsigned)((w.npaths + 255) / 256)), dim3(256), 0, 0, sc, w,
                           dcand.ptr, dcount.ptr);
        MPSS_HIP(hipGetLastError());
        MPSS_HIP(hipMemcpy(cnt.data(), dcount.ptr, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
        MPSS_HIP(hipMemcpy(cand.data(), dcand.ptr, sizeof(SurfacePoint) * cand.size(), hipMemcpyDeviceToHost));
        state = accept.consume(cand.data(), cnt.data(), kBatch, kBatchesPerLaunch, kPoissonCand);
    }
    if (state == PoissonAccept::State::GaveUp) {
        fprintf(stderr, "mpss: Warning: There don't seem to be any objects with BSSRDFs in this scene. "
                        "Giving up.\n");
        return;
    }
    points_ = std::move(accept.points);
}

}  // namespace mpss
