// scene_upload.hip -- the scene of the per-pixel path: the host scene's mutators (meshes, lights, camera)
// and its device copy (upload_scene and its steps, upload_materials, render_scene).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"
#include "envmap.h"
#include "render.h"
#include "spectral.h"
#include "texture_build.h"

namespace mpss {

namespace {
float det3(const float *m) {
    return m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) +
           m[2] * (m[4] * m[9] - m[5] * m[8]);
}
int bvh_depth(const std::vector<BvhNode> &n, int i) {
    if (n[i].nprims > 0) return 1;
    return 1 + std::max(bvh_depth(n, i + 1), bvh_depth(n, n[i].offset));
}
// A new light's sample count, after the checks both kinds share: "nsamples" quartered under quickrender
// (CreateDiffuseAreaLight, CreateInfiniteLight). who: the caller's name in the error messages.
int light_nsamples(const char *who, int nsamples, size_t nlights, bool quick_render) {
    if (nsamples < 1) throw Error(MPSS_ERR_INVALID, std::string(who) + ": nsamples must be >= 1");
    if (nlights >= 254) throw Error(MPSS_ERR_INVALID, std::string(who) + ": at most 254 lights");
    return quick_render ? std::max(1, nsamples / 4) : nsamples;
}
}  // namespace

void Context::add_mesh(uint32_t nv, const float *P, const float *N, const float *S, const float *uv, uint32_t nt,
                       const int32_t *idx, const float *o2w, const float *w2o, bool reverse, uint32_t material) {
    std::lock_guard<std::mutex> g(mu_);
    if (material >= materials_.size()) throw Error(MPSS_ERR_INVALID, "add_mesh: unknown material id");
    if (materials_[material]->dipole)
        throw Error(MPSS_ERR_INVALID, "add_mesh: a dipole material is an Rd functor for mpss_mo_batch, not a surface");
    Mesh m;
    m.P.assign(P, P + 3 * (size_t)nv);
    if (N) m.N.assign(N, N + 3 * (size_t)nv);
    if (S) m.S.assign(S, S + 3 * (size_t)nv);
    if (uv) m.uv.assign(uv, uv + 2 * (size_t)nv);
    m.idx.assign(idx, idx + 3 * (size_t)nt);
    for (uint32_t i = 0; i < 3 * nt; ++i)
        if (m.idx[i] < 0 || (uint32_t)m.idx[i] >= nv) throw Error(MPSS_ERR_INVALID, "add_mesh: vertex index out of range");
    memcpy(m.o2w, o2w, sizeof(m.o2w));
    memcpy(m.w2o, w2o, sizeof(m.w2o));
    m.material = material;
    m.reverse_orientation = reverse;
    m.swaps_handedness = det3(o2w) < 0.f;  // Transform::SwapsHandedness
    scene_.meshes.push_back(std::move(m));
    mark_scene_dirty_locked();
}

void Context::add_sphere_light(const float *c, float r, const float *Lemit, int nsamples) {
    std::lock_guard<std::mutex> g(mu_);
    if (!(r > 0.f)) throw Error(MPSS_ERR_INVALID, "add_sphere_light: radius must be positive");
    SceneLight l;
    l.nsamples = light_nsamples("add_sphere_light", nsamples, scene_.lights.size(), cfg_.quick_render);
    memcpy(l.center, c, sizeof(l.center));
    l.radius = r;
    memcpy(l.Lemit, Lemit, sizeof(l.Lemit));
    scene_.lights.push_back(l);
    mark_scene_dirty_locked();
}

// CreateInfiniteLight + the InfiniteAreaLight ctor without a map (lights/infinite.cpp:66-90,
// 180-188): texels[0] = L.ToRGBSpectrum(); Le and Sample_L convert map lookups back with
// Spectrum(rgb, SPECTRUM_ILLUMINANT) on the device (spectrum_tables.h).
void Context::add_infinite_light(const float *L, int nsamples, const float *l2w, const float *w2l, int W, int H,
                                 const float *texels) {
    std::lock_guard<std::mutex> g(mu_);
    SceneLight l;
    l.nsamples = light_nsamples("add_infinite_light", nsamples, scene_.lights.size(), cfg_.quick_render);
    if (texels && (W < 1 || H < 1 || (int64_t)W * H > (int64_t)1 << 28))
        throw Error(MPSS_ERR_INVALID, "add_infinite_light: bad map resolution");
    l.kind = 1;
    l.center[0] = l.center[1] = l.center[2] = 0.f;
    l.radius = 0.f;
    memcpy(l.Lemit, L, sizeof(l.Lemit));
    float rgb[3];
    spectrum_to_rgb(L, rgb);  // L.ToRGBSpectrum()
    if (texels) {             // texels[i] *= L.ToRGBSpectrum()
        l.map_w = W;
        l.map_h = H;
        l.map.resize((size_t)W * H * 3);
        for (size_t i = 0; i < (size_t)W * H; ++i)
            for (int k = 0; k < 3; ++k) l.map[3 * i + k] = texels[3 * i + k] * rgb[k];
    } else {
        l.map_w = l.map_h = 1;
        l.map.assign(rgb, rgb + 3);
    }
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            l.l2w[3 * r + k] = l2w[4 * r + k];
            l.w2l[3 * r + k] = w2l[4 * r + k];
        }
    scene_.lights.push_back(std::move(l));
    mark_scene_dirty_locked();
}

void Context::set_camera(const float *r2c, const float *c2w, int xres, int yres) {
    std::lock_guard<std::mutex> g(mu_);
    if (xres <= 0 || yres <= 0) throw Error(MPSS_ERR_INVALID, "set_camera: bad resolution");
    memcpy(scene_.camera.raster_to_camera, r2c, sizeof(float) * 16);
    memcpy(scene_.camera.camera_to_world, c2w, sizeof(float) * 16);
    scene_.camera.xres = xres;
    scene_.camera.yres = yres;
    mark_scene_dirty_locked();
}

void Context::upload_scene() {
    activate();
    quiesce_locked();  // the scene buffers in-flight renders read are about to be replaced
    if (scene_.meshes.empty()) throw Error(MPSS_ERR_INVALID, "scene has no meshes");
    upload_bvh();
    upload_camera_bins();
    upload_meshes();
    upload_lights();
    ++scene_gen_;  // the workspaces' replay cursors belong to the old scene
    ++n_scene_uploads_;
    upload_textures();
    upload_materials();
    scene_dirty_ = false;
}

// the BVH over every mesh's triangles, plain and threaded (scene_plain.h thread_bvh), and the triangles
// in its leaf order
void Context::upload_bvh() {
    build_bvh(scene_);
    const int depth = bvh_depth(scene_.bvh, 0);
    if (depth > 47) throw Error(MPSS_ERR_INTERNAL, "BVH deeper than the 48-entry traversal stack");
    d_bvh_.upload(scene_.bvh.data(), scene_.bvh.size());
    const std::vector<BvhNode> th = thread_bvh(scene_.bvh);
    d_bvh_thread_.upload(th.data(), th.size());
    d_tris_.upload(scene_.tris.data(), scene_.tris.size());
}

// reference sampler: the camera rays' candidate triangles per pixel (scene.h CameraBins)
void Context::upload_camera_bins() {
    if (cfg_.sampler == MPSS_SAMPLER_REFERENCE && scene_.camera.xres > 0) {
        CameraBins b;
        build_camera_bins(scene_, b);
        d_bin_off_.upload(b.off.data(), b.off.size());
        d_bin_tri_.upload(b.tri.data(), b.tri.size());
        d_bin_all_.upload(b.all.data(), b.all.size());
        bin_w_ = b.w;
        bin_nall_ = (int)b.all.size();
    }
}

// the triangle -> mesh maps, every mesh's vertex arrays, and the RenderMesh records over them
void Context::upload_meshes() {
    d_tri_mesh_.upload(scene_.tri_mesh.data(), scene_.tri_mesh.size());
    d_tri_local_.upload(scene_.tri_local.data(), scene_.tri_local.size());
    d_mesh_bufs_.clear();
    std::vector<RenderMesh> rm;
    for (const Mesh &m : scene_.meshes) {
        auto add = [&](const std::vector<float> &v) -> const float * {
            if (v.empty()) return nullptr;
            d_mesh_bufs_.emplace_back(new DevBuf<float>());
            d_mesh_bufs_.back()->upload(v.data(), v.size());
            return d_mesh_bufs_.back()->ptr;
        };
        RenderMesh r{};
        r.view.P = add(m.P);
        r.view.N = add(m.N);
        r.view.S = add(m.S);
        r.view.uv = add(m.uv);
        std::vector<float> idxf(m.idx.size());
        memcpy(idxf.data(), m.idx.data(), sizeof(int32_t) * m.idx.size());
        r.view.idx = reinterpret_cast<const int32_t *>(add(idxf));
        memcpy(r.view.o2w_store, m.o2w, sizeof(m.o2w));
        memcpy(r.view.w2o_store, m.w2o, sizeof(m.w2o));
        r.view.flip = (int)(m.reverse_orientation ^ m.swaps_handedness);
        r.material = m.material;
        rm.push_back(r);
    }
    // matrices live inside the device-side RenderMesh records; fix up their pointers there
    d_meshes_.alloc(rm.size());
    for (size_t i = 0; i < rm.size(); ++i) {
        rm[i].view.o2w = reinterpret_cast<float *>(reinterpret_cast<char *>(d_meshes_.ptr + i) +
                                                   offsetof(RenderMesh, view) + offsetof(MeshView, o2w_store));
        rm[i].view.w2o = reinterpret_cast<float *>(reinterpret_cast<char *>(d_meshes_.ptr + i) +
                                                   offsetof(RenderMesh, view) + offsetof(MeshView, w2o_store));
    }
    d_meshes_.upload(rm.data(), rm.size());
}

// the RenderLight records, an infinite light's maps in one device block each (envmap.h), and the
// lights' places in a replay-table row (replay_k_)
void Context::upload_lights() {
    std::vector<RenderLight> rl;
    int replay_off = kReplayImage;
    d_envmaps_.clear();
    // every light's map pointers address valid memory (a 1x1 zero map for area lights), so no
    // load the compiler hoists out of a kind test can fault
    if (!d_zero_map_.ptr) {
        const float z[16] = {};
        d_zero_map_.upload(z, 16);
    }
    for (const SceneLight &l : scene_.lights) {
        RenderLight r{};
        r.s = full_sphere(V3{l.center[0], l.center[1], l.center[2]}, l.radius);
        memcpy(r.Lemit, l.Lemit, sizeof(r.Lemit));
        r.kind = l.kind;
        r.tw = r.th = r.nu = r.nv = 1;
        r.tex = r.func = r.cdf = r.rint = r.mcdf = d_zero_map_.ptr;
        if (l.kind == 1) {  // radiance MIPMap level 0 + Distribution2D, one device block per light
            memcpy(r.l2w, l.l2w, sizeof(r.l2w));
            memcpy(r.w2l, l.w2l, sizeof(r.w2l));
            const EnvMap em = build_envmap(l.map_w, l.map_h, l.map.data());
            std::vector<float> blk;
            const size_t o_tex = blk.size();
            blk.insert(blk.end(), em.tex.begin(), em.tex.end());
            const size_t o_func = blk.size();
            blk.insert(blk.end(), em.func.begin(), em.func.end());
            const size_t o_cdf = blk.size();
            blk.insert(blk.end(), em.cdf.begin(), em.cdf.end());
            const size_t o_rint = blk.size();
            blk.insert(blk.end(), em.row_int.begin(), em.row_int.end());
            const size_t o_mcdf = blk.size();
            blk.insert(blk.end(), em.mcdf.begin(), em.mcdf.end());
            d_envmaps_.emplace_back(new DevBuf<float>());
            DevBuf<float> &db = *d_envmaps_.back();
            db.upload(blk.data(), blk.size());
            r.tw = em.w0;
            r.th = em.h0;
            r.nu = em.nu;
            r.nv = em.nv;
            r.tex = db.ptr + o_tex;
            r.func = db.ptr + o_func;
            r.cdf = db.ptr + o_cdf;
            r.rint = db.ptr + o_rint;
            r.mcdf = db.ptr + o_mcdf;
            r.mint = em.mint;
            r.s.r = 0.f;
        }
        // RoundUpPow2(nSamples) and LDSampler::RoundSize(nSamples) are one value (render.h RenderLight)
        r.nsamples_pow2 = r.nsamples_round = replay_round_up_pow2(l.nsamples);
        r.replay_off = replay_off;
        replay_off += kReplayPerLightSample * r.nsamples_round;
        rl.push_back(r);
    }
    d_lights_.upload(rl.data(), rl.size());
    replay_k_ = replay_off;
}

// the EWA weight table and the textures' pyramids, once each
void Context::upload_textures() {
    if (!d_lut_.ptr) d_lut_.upload(ewa_weight_lut(), kEwaLut);
    for (auto &t : textures_)
        if (!t->dev.ptr) t->dev.upload(t->py.data.data(), t->py.data.size());
}

// The RenderMaterial records (d_materials_) from materials_: the whole of the device scene that a
// material's parameters reach. The textures they view are on the device already (upload_scene: binding
// or adding one marks the scene dirty).
void Context::upload_materials() {
    activate();
    quiesce_locked();  // in-flight renders read d_materials_
    std::vector<RenderMaterial> rmat;
    for (const auto &mp : materials_) {
        const Material &m = *mp;
        RenderMaterial r{};
        memcpy(r.R, m.Kr, sizeof(r.R));
        bool black = true;
        for (int c = 0; c < NB; ++c) black = black && m.Kr[c] == 0.f;
        r.has_refl = !black;
        r.r_lo = INFINITY;
        r.r_hi = 0.f;
        r.r_nonneg = 1;
        for (int c = 0; c < NB; ++c) {
            if (!(m.Kr[c] >= 0.f)) r.r_nonneg = 0;
            if (m.Kr[c] > 0.f) r.r_lo = std::min(r.r_lo, m.Kr[c]);
            r.r_hi = std::max(r.r_hi, m.Kr[c]);
        }
        if (black) r.r_lo = 0.f;
        memcpy(r.T, m.Kt, sizeof(r.T));
        bool tblack = true;
        for (int c = 0; c < NB; ++c) tblack = tblack && m.Kt[c] == 0.f;
        r.has_trans = !tblack;
        for (int c = 0; c < NB; ++c) {
            r.alb_mix[c] = m_pow(m.albedo[c], cfg_.mix);
            r.alb_1mmix[c] = m_pow(m.albedo[c], 1.f - cfg_.mix);
        }
        const float rough = m.roughness < 1e-3f ? 1e-3f : m.roughness;
        r.mf.rms2 = rough * rough;
        r.mf.rcp_rms2 = 1 / r.mf.rms2;
        r.mf.eta = m.ior;
        r.mf.fixed_fresnel = m.double_ref_sslf ? 1 : 0;
        r.rho = m.dev_rho.ptr;
        r.n_rho = (int)m.rho.hd.size();
        r.has_bssrdf = m.no_bssrdf ? 0 : 1;
        r.is_mc = m.is_monte_carlo ? 1 : 0;
        r.mix = cfg_.mix;
        for (int c = 0; c < NB; ++c) r.band_pos[c] = m.dev_profile.groups.pos[c];
        if (m.albedo_tex >= 0) {
            r.has_alb_tex = 1;
            r.alb_tex = textures_[m.albedo_tex]->device_view(d_lut_.ptr);
        }
        if (m.bump_tex >= 0) {
            r.has_bump = 1;
            r.bump_tex = textures_[m.bump_tex]->device_view(d_lut_.ptr);
        }
        if (m.kr_tex >= 0) {
            r.has_kr_tex = 1;
            r.kr_tex = textures_[m.kr_tex]->device_view(d_lut_.ptr);
        }
        if (m.kt_tex >= 0) {
            r.has_kt_tex = 1;
            r.kt_tex = textures_[m.kt_tex]->device_view(d_lut_.ptr);
        }
        rmat.push_back(r);
    }
    d_materials_.upload(rmat.data(), rmat.size());
    materials_dirty_ = false;
}

RenderScene Context::render_scene() const {
    RenderScene sc{};
    sc.bvh = d_bvh_.ptr;
    sc.bvh_thread = d_bvh_thread_.ptr;
    sc.nbvh = (int)scene_.bvh.size();
    sc.tris = d_tris_.ptr;
    sc.tri_mesh = d_tri_mesh_.ptr;
    sc.tri_local = d_tri_local_.ptr;
    sc.meshes = d_meshes_.ptr;
    sc.lights = d_lights_.ptr;
    sc.materials = d_materials_.ptr;
    sc.nlights = (int)scene_.lights.size();
    for (const SceneLight &l : scene_.lights) sc.n_infinite += l.kind == 1;
    sc.nmaterials = (int)materials_.size();
    sc.xres = scene_.camera.xres;
    sc.yres = scene_.camera.yres;
    memcpy(sc.raster_to_camera, scene_.camera.raster_to_camera, sizeof(sc.raster_to_camera));
    memcpy(sc.camera_to_world, scene_.camera.camera_to_world, sizeof(sc.camera_to_world));
    // dxCamera = RasterToCamera(Point(1,0,0)) - RasterToCamera(Point(0,0,0)) (perspective.cpp:47-48)
    const V3 c0 = xform_point(sc.raster_to_camera, V3{0.f, 0.f, 0.f});
    const V3 dx = xform_point(sc.raster_to_camera, V3{1.f, 0.f, 0.f}) - c0;
    const V3 dy = xform_point(sc.raster_to_camera, V3{0.f, 1.f, 0.f}) - c0;
    sc.dx_camera[0] = dx.x;
    sc.dx_camera[1] = dx.y;
    sc.dx_camera[2] = dx.z;
    sc.dy_camera[0] = dy.x;
    sc.dy_camera[1] = dy.y;
    sc.dy_camera[2] = dy.z;
    for (const auto &m : materials_) sc.any_tex |= (m->albedo_tex >= 0 || m->bump_tex >= 0);
    for (const auto &m : materials_) sc.any_spec_tex |= (m->kr_tex >= 0 || m->kt_tex >= 0);
    return sc;
}

}  // namespace mpss
