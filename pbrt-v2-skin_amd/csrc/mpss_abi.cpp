// mpss_abi.cpp -- the extern "C" boundary of libmpss (include/mpss.h).
#include <algorithm>
#include <atomic>
#include <thread>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mpss.h"
#include "common_grid.h"
#include "context.h"
#include "material.h"
#include "mc_profile.h"
#include "mo_kernel.h"
#include "profile_fit.h"
#include "sog_fit.h"
#include "spectral.h"

using namespace mpss;

namespace {
thread_local std::string g_last_error;

template <class F>
int guarded(F &&fn) {
    try {
        fn();
        return MPSS_OK;
    } catch (const Error &e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc &) {
        g_last_error = "out of memory";
        return MPSS_ERR_NOMEM;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return MPSS_ERR_INTERNAL;
    } catch (...) {
        g_last_error = "unknown error";
        return MPSS_ERR_INTERNAL;
    }
}

void require(bool ok, const char *msg) {
    if (!ok) throw Error(MPSS_ERR_INVALID, msg);
}

// DoProfileFit's setup (profilefit.cpp:284-312): sorted ranges, the sigma list over the whole grid, the
// clipped id range
struct FitPlan {
    std::vector<float> range[4];
    uint32_t n[4];
    uint32_t total = 0, id0 = 0, id1 = 0;
    std::vector<float> sigmas;
    void params(uint32_t id, float out[4]) const {
        const float *const r[4] = {range[0].data(), range[1].data(), range[2].data(), range[3].data()};
        fit_params_from_id(id, r, n, out);
    }
};

FitPlan make_fit_plan(const mpss_profilefit &f, bool with_sigmas = true) {
    FitPlan pl;
    const float *src[4] = {f.f_mel, f.f_eu, f.f_blood, f.f_ohg};
    const uint32_t cnt[4] = {f.n_f_mel, f.n_f_eu, f.n_f_blood, f.n_f_ohg};
    uint64_t total = 1;
    for (int k = 0; k < 4; ++k) {
        require(src[k] && cnt[k] >= 1, "profile fit: each of f_mel, f_eu, f_blood, f_ohg needs at least one value");
        pl.range[k].assign(src[k], src[k] + cnt[k]);
        std::sort(pl.range[k].begin(), pl.range[k].end());  // FindParamRange
        pl.n[k] = cnt[k];
        total *= cnt[k];
        require(total <= (1u << 20), "profile fit: more than 2^20 combinations");
    }
    require(f.desired_length >= 2 && f.desired_length <= 1024, "profile fit: desired_length outside 2..1024");
    for (int l = 0; l < 2; ++l)
        require(f.layer_thickness_nm[l] > 0.f && f.layer_ior[l] > 0.f, "profile fit: layers need thickness and ior > 0");
    pl.total = (uint32_t)total;
    float mfp_min = INFINITY, mfp_max = 0.f;
    for (uint32_t id = 0; with_sigmas && id < pl.total; ++id) {
        float v[4];
        pl.params(id, v);
        skin_fit_mfp_range(v[0], v[1], v[2], v[3], mfp_min, mfp_max);
    }
    if (with_sigmas) pl.sigmas = fit_sigma_list(mfp_min, mfp_max);
    pl.id0 = (uint32_t)std::max(0, f.id_min);
    pl.id1 = f.id_max < 0 ? pl.total : (uint32_t)std::min<int64_t>(pl.total, f.id_max);
    if (pl.id1 < pl.id0) pl.id1 = pl.id0;
    return pl;
}

// the layers of ids [id0, id1) in millimetres and every channel's own mfp bounds (GaussianFitTask::Run :165-173)
void fit_layers(const mpss_profilefit &f, const FitPlan &pl, std::vector<LayerParams> &lp, std::vector<float> &mfp_min,
                std::vector<float> &mfp_max) {
    const uint32_t n = pl.id1 - pl.id0;
    lp.resize(n);
    mfp_min.resize((size_t)n * NB);
    mfp_max.resize((size_t)n * NB);
    for (uint32_t i = 0; i < n; ++i) {
        float v[4];
        pl.params(pl.id0 + i, v);
        skin_fit_layer_params(v[0], v[1], v[2], v[3], f.layer_thickness_nm, f.layer_ior, lp[i]);
        for (int sc = 0; sc < NB; ++sc) {
            float lo = INFINITY, hi = 0.f;
            for (int l = 0; l < 2; ++l) {
                const float mfp = 1.f / (lp[i].mua[l][sc] + lp[i].musp[l][sc]);
                lo = std::min(lo, mfp);
                hi = std::max(hi, mfp);
            }
            mfp_min[(size_t)i * NB + sc] = lo;
            mfp_max[(size_t)i * NB + sc] = hi;
        }
    }
}

void fit_rgb_rows(uint32_t n_ids, uint32_t ns, const float *coeffs, float *rgb) {
    for (uint32_t i = 0; i < n_ids; ++i)
        for (uint32_t s = 0; s < ns; ++s) {
            float spec[NB], out[3];
            for (int sc = 0; sc < NB; ++sc) spec[sc] = coeffs[((size_t)i * NB + sc) * ns + s];
            spectrum_to_rgb(spec, out);
            for (int k = 0; k < 3; ++k) rgb[((size_t)i * 3 + k) * ns + s] = out[k];
        }
}

void fit_no_candidate(const FitPlan &pl, int64_t profile) {
    throw Error(MPSS_ERR_INTERNAL, "profile fit: id " + std::to_string(pl.id0 + profile / NB) + " band " +
                                       std::to_string(profile % NB) +
                                       " has no candidate window (no sigma within [mfpMin / 2, mfpMax * 2] "
                                       "with a full window around it)");
}
}  // namespace

extern "C" {

int mpss_abi_version(void) { return 13; }  // 2: poisson point finder, infinite lights; 3: imagemap textures;
                                          // 4: tile costs, wave-iteration stats, thread-safe calls;
                                          // 5: reference-sampler replay, dipole materials;
                                          // 6: GPU octree build (octree_on_host), mpss_octree_export;
                                          // 7: gather choices in mpss_config (mo_band_dealing,
                                          //    mo_work_stealing, mo_near_field), count_traversal 2;
                                          // 8: light spheres seen directly shaded (default matte),
                                          //    rebuilds wait for in-flight render / mo_batch calls;
                                          // 9: GPU tessellation (tessellate_on_host), size bounds
                                          // 10: mo_common_grid, mpss_get_gather_info, common-grid
                                          //     lane-record counts in mpss_render_stats
                                          // 11: rgbprofile through the sharded gather (its own common
                                          //     grid), mpss_host_common_grid u1start / rgb mode
                                          // 12: LayeredSkin genprofile / showirradiancepoints /
                                          //     irradiancepointsize; mpss_host_common_grid near_field
                                          // 13: per-group, per-path L2 footprint in mpss_render_stats;
                                          //     common-grid rows H steps apart past ua, bad cells
                                          //     flagged (mpss_host_common_grid ua / hinv)
const char *mpss_last_error(void) { return g_last_error.c_str(); }

void mpss_config_defaults(mpss_config *c) {
    if (!c) return;
    c->device = 0;
    c->max_depth = 5;
    c->max_error = .05f;
    c->min_sample_distance = .25f;
    c->mix = .5f;
    c->show_irradiance_points = 0;
    c->incenter = 0;
    c->quick_render = 0;
    c->exact_mo = 0;
    c->kernel_timing = 0;
    c->count_traversal = 0;
    c->profile_on_host = 0;
    c->max_batch_samples = (int64_t)1 << 26;
    c->use_poisson_point_finder = 0;
    c->sampler = MPSS_SAMPLER_HASH;
    c->replay_cores = 8;
    c->octree_on_host = 0;
    c->mo_band_dealing = 0;
    c->mo_work_stealing = 1;
    c->mo_near_field = 5088;
    c->tessellate_on_host = 0;
    c->mo_common_grid = 1;
}

int mpss_create(const mpss_config *cfg, mpss_ctx **out) {
    return guarded([&] {
        require(cfg && out, "mpss_create: null argument");
        *out = nullptr;
        auto ctx = std::make_unique<Context>(*cfg);
        *out = reinterpret_cast<mpss_ctx *>(ctx.release());
    });
}

void mpss_destroy(mpss_ctx *ctx) { delete reinterpret_cast<Context *>(ctx); }

void mpss_layeredskin_defaults(mpss_layeredskin *m) {
    if (!m) return;
    m->roughness = 0.4f;
    m->nmperunit = 100e6f;
    m->f_mel = 0.15f;
    m->f_eu = 1.f;
    m->f_blood = 0.002f;
    m->f_ohg = 0.3f;
    m->ga_epi = 0.9f;
    m->ga_derm = 0.8f;
    m->b_derm = 0.4f;
    m->layer_thickness_nm[0] = 0.25e6f;
    m->layer_thickness_nm[1] = 20e6f;
    m->layer_ior[0] = m->layer_ior[1] = 1.4f;
    for (int i = 0; i < MPSS_NBANDS; ++i) m->albedo[i] = m->Kr[i] = m->Kt[i] = 1.f;
    m->desired_length = 512;
    m->lerp_on_thin_slab = 1;
    m->double_ref_sslf = 0;
    m->use_monte_carlo = 0;
    m->photons = 10000000ull;
    m->rgb_profile = 0;
    m->gen_profile = 1;
    m->show_irradiance_points = 0;
    m->irradiance_point_size = 0.002f;
}

int mpss_add_layeredskin(mpss_ctx *c, const mpss_layeredskin *m, uint32_t *id) {
    return guarded([&] {
        require(c && m && id, "mpss_add_layeredskin: null argument");
        require(m->desired_length >= 2 && m->desired_length <= 4096, "desiredlength out of range [2, 4096]");
        require(m->nmperunit > 0.f, "nmperunit must be positive");
        require(!m->show_irradiance_points || m->irradiance_point_size > 0.f,
                "irradiancepointsize must be positive with showirradiancepoints");
        *id = reinterpret_cast<Context *>(c)->add_layeredskin(*m);
    });
}

int mpss_update_layeredskin(mpss_ctx *c, uint32_t id, const mpss_layeredskin *m) {
    return guarded([&] {
        require(c && m, "mpss_update_layeredskin: null argument");
        require(m->desired_length >= 2 && m->desired_length <= 4096, "desiredlength out of range [2, 4096]");
        require(m->nmperunit > 0.f, "nmperunit must be positive");
        require(!m->show_irradiance_points || m->irradiance_point_size > 0.f,
                "irradiancepointsize must be positive with showirradiancepoints");
        reinterpret_cast<Context *>(c)->update_layeredskin(id, *m);
    });
}

int mpss_build_counts(mpss_ctx *c, uint64_t counts[4]) {
    return guarded([&] {
        require(c && counts, "mpss_build_counts: null argument");
        reinterpret_cast<Context *>(c)->build_counts(counts);
    });
}

void mpss_imagemap_defaults(mpss_imagemap *t) {
    if (!t) return;
    memset(t, 0, sizeof(*t));
    t->scale = 1.f;
    t->gamma = 1.f;
    t->max_anisotropy = 8.f;
    t->uscale = t->vscale = 1.f;
}

int mpss_add_imagemap(mpss_ctx *c, const mpss_imagemap *t, uint32_t *id) {
    return guarded([&] {
        require(c && t && id, "mpss_add_imagemap: null argument");
        *id = reinterpret_cast<Context *>(c)->add_imagemap(*t);
    });
}

int mpss_set_material_textures(mpss_ctx *c, uint32_t mid, int32_t albedo, int32_t bump) {
    return guarded([&] {
        require(c != nullptr, "mpss_set_material_textures: null context");
        reinterpret_cast<Context *>(c)->set_material_textures(mid, albedo, bump);
    });
}

int mpss_set_material_tables(mpss_ctx *c, const float *rd, uint32_t len, const float *rcp, const float *rho,
                             uint32_t n_rho, const float *albedo, int is_mc, uint32_t *id) {
    return guarded([&] {
        require(c && rd && rcp && rho && id, "mpss_set_material_tables: null argument");
        require(len >= 2 && n_rho >= 2, "tables need at least 2 entries");
        *id = reinterpret_cast<Context *>(c)->set_material_tables(rd, len, rcp, rho, n_rho, albedo, is_mc != 0);
    });
}

int mpss_add_dipole_material(mpss_ctx *c, const float *sigma_a, const float *sigmap_s, float eta, uint32_t *id) {
    return guarded([&] {
        require(c && sigma_a && sigmap_s && id, "mpss_add_dipole_material: null argument");
        require(eta > 0.f, "mpss_add_dipole_material: eta must be positive");
        *id = reinterpret_cast<Context *>(c)->add_dipole_material(sigma_a, sigmap_s, eta);
    });
}

int mpss_get_material_tables(mpss_ctx *c, uint32_t id, float *rd, uint32_t *len, float *rcp, float *rho,
                             uint32_t *n_rho, float *total) {
    return guarded([&] {
        require(c && len && n_rho, "mpss_get_material_tables: null argument");
        reinterpret_cast<Context *>(c)->material_tables(id, rd, len, rcp, rho, n_rho, total);
    });
}

int mpss_host_common_grid(const float *table, uint32_t L, const float *rcp, int snake, int near_field, float *rows,
                          uint32_t *n_rows, int32_t *bands, float *rg, float *u0lim, float *u1lim, float *u1start,
                          uint32_t *row0, uint32_t *ubase, float *rel_err, float *l1_err, float *ua, float *hinv,
                          int *ok) {
    return guarded([&] {
        require(table && rcp && ok, "mpss_host_common_grid: null argument");
        require(L >= 2 && L < (1u << 24), "mpss_host_common_grid: L out of range");
        require(snake >= 0 && snake <= 2, "mpss_host_common_grid: snake must be 0, 1 or 2");
        require(near_field == 10236 || near_field == 5088, "mpss_host_common_grid: near_field must be 10236 or 5088");
        BandGroups g = make_band_groups(rcp, snake == 1);
        if (snake == 2)  // rgbprofile: rows 0..2 (R, G, B) in every group (DeviceProfile::set_rgb)
            for (int k = 0; k < kGroups; ++k)
                for (int j = 0; j < 4; ++j) g.band[k][j] = j < 3 ? j : -1;
        CommonGrid cg;
        std::vector<float4> h;
        float rel[NB], l1[NB];
        *ok = build_common_grid(table, (int)L, rcp, g, cg, h, rel, l1, near_field, snake == 2 ? 28 : 0, snake == 2) ? 1 : 0;
        if (n_rows) {
            if (rows) require(*n_rows >= h.size() / 2, "mpss_host_common_grid: rows too small");
            *n_rows = (uint32_t)(h.size() / 2);
        }
        if (rows) memcpy(rows, h.data(), sizeof(float4) * h.size());
        for (int k = 0; k < kGroups; ++k) {
            for (int j = 0; j < 4; ++j)
                if (bands) bands[4 * k + j] = g.band[k][j];
            if (rg) rg[k] = cg.rg[k];
            if (u0lim) u0lim[k] = cg.u0lim[k];
            if (u1lim) u1lim[k] = cg.u1lim[k];
            if (u1start) u1start[k] = cg.u1start[k];
            if (row0) row0[k] = cg.row0[k];
            if (ubase) ubase[k] = cg.ubase[k];
            if (ua) ua[k] = cg.ua[k];
            if (hinv) hinv[k] = cg.hinv[k];
        }
        for (int c = 0; c < NB; ++c) {
            if (rel_err) rel_err[c] = rel[c];
            if (l1_err) l1_err[c] = l1[c];
        }
    });
}

int mpss_get_common_grid(mpss_ctx *c, uint32_t id, int near_field, float *rows, uint32_t *n_rows, int32_t *bands,
                         float *rg, float *u0lim, float *u1lim, float *u1start, uint32_t *row0, uint32_t *ubase,
                         float *rel_err, float *l1_err, float *ua, float *hinv, int *ok) {
    return guarded([&] {
        require(c && ok, "mpss_get_common_grid: null argument");
        require(near_field == 10236 || near_field == 5088, "mpss_get_common_grid: near_field must be 10236 or 5088");
        reinterpret_cast<Context *>(c)->common_grid(id, near_field, rows, n_rows, bands, rg, u0lim, u1lim, u1start, row0,
                                                    ubase, rel_err, l1_err, ua, hinv, ok);
    });
}

int mpss_get_gather_info(mpss_ctx *c, uint32_t id, int *common_grid, float *rel_err, float *l1_err) {
    return guarded([&] {
        require(c && common_grid, "mpss_get_gather_info: null argument");
        reinterpret_cast<Context *>(c)->gather_info(id, common_grid, rel_err, l1_err);
    });
}

int mpss_set_irradiance_points(mpss_ctx *c, uint32_t n, const float *p, const float *nrm, const float *E,
                               const float *area) {
    return guarded([&] {
        require(c && p && nrm && E && area, "mpss_set_irradiance_points: null argument");
        require(n > 0, "mpss_set_irradiance_points: empty point set");
        require(n <= (1u << 30), "mpss_set_irradiance_points: at most 2^30 points");
        reinterpret_cast<Context *>(c)->set_irradiance_points((int)n, p, nrm, E, area);
    });
}

int mpss_octree_info(mpss_ctx *c, uint32_t *nn, uint32_t *md, uint32_t *np) {
    return guarded([&] {
        require(c, "mpss_octree_info: null ctx");
        const DeviceOctree &t = reinterpret_cast<Context *>(c)->octree();
        if (nn) *nn = (uint32_t)t.n_nodes;
        if (md) *md = (uint32_t)t.max_depth;
        if (np) *np = (uint32_t)t.n_points;
    });
}

int mpss_octree_export(mpss_ctx *c, void *nodes, float *node_et, float *pt_hdr, float *pt_e, int32_t *pt_index) {
    return guarded([&] {
        require(c, "mpss_octree_export: null ctx");
        reinterpret_cast<Context *>(c)->export_octree(nodes, node_et, pt_hdr, pt_e, pt_index);
    });
}

int mpss_mo_batch(mpss_ctx *c, uint32_t id, uint32_t q, const float *p_dev, float *mo_dev, int32_t *counters_dev,
                  void *stream) {
    return guarded([&] {
        require(c && (q == 0 || (p_dev && mo_dev)), "mpss_mo_batch: null argument");
        require(q <= (1u << 30), "mpss_mo_batch: at most 2^30 queries per call");
        reinterpret_cast<Context *>(c)->mo_batch(id, (int)q, p_dev, mo_dev, counters_dev, (hipStream_t)stream);
    });
}

int mpss_add_mesh(mpss_ctx *c, uint32_t nv, const float *P, const float *N, const float *S, const float *uv,
                  uint32_t nt, const int32_t *idx, const float *o2w, const float *w2o, int rev, uint32_t mat) {
    return guarded([&] {
        require(c && P && idx && o2w && w2o && nv > 0 && nt > 0, "mpss_add_mesh: bad argument");
        reinterpret_cast<Context *>(c)->add_mesh(nv, P, N, S, uv, nt, idx, o2w, w2o, rev != 0, mat);
    });
}

int mpss_add_sphere_light(mpss_ctx *c, const float *center, float r, const float *L, int ns) {
    return guarded([&] {
        require(c && center && L, "mpss_add_sphere_light: null argument");
        reinterpret_cast<Context *>(c)->add_sphere_light(center, r, L, ns);
    });
}

int mpss_add_infinite_light(mpss_ctx *c, const float *L, int ns, const float *l2w, const float *w2l) {
    return guarded([&] {
        require(c && L && l2w && w2l, "mpss_add_infinite_light: null argument");
        reinterpret_cast<Context *>(c)->add_infinite_light(L, ns, l2w, w2l);
    });
}

int mpss_add_infinite_light_map(mpss_ctx *c, const float *L, int ns, const float *l2w, const float *w2l, int w, int h,
                                const float *texels) {
    return guarded([&] {
        require(c && L && l2w && w2l && texels, "mpss_add_infinite_light_map: null argument");
        reinterpret_cast<Context *>(c)->add_infinite_light(L, ns, l2w, w2l, w, h, texels);
    });
}

int mpss_set_camera(mpss_ctx *c, const float *r2c, const float *c2w, int xres, int yres) {
    return guarded([&] {
        require(c && r2c && c2w, "mpss_set_camera: null argument");
        reinterpret_cast<Context *>(c)->set_camera(r2c, c2w, xres, yres);
    });
}

int mpss_set_surface_points(mpss_ctx *c, uint32_t n, const void *rec) {
    return guarded([&] {
        require(c && (n == 0 || rec), "mpss_set_surface_points: null argument");
        reinterpret_cast<Context *>(c)->set_surface_points(n, reinterpret_cast<const SurfacePoint *>(rec));
    });
}

int mpss_get_surface_points(mpss_ctx *c, void *rec, uint32_t *n) {
    return guarded([&] {
        require(c && n, "mpss_get_surface_points: null argument");
        const auto v = reinterpret_cast<Context *>(c)->surface_points();
        *n = (uint32_t)v.size();
        if (rec) memcpy(rec, v.data(), sizeof(SurfacePoint) * v.size());
    });
}

int mpss_load_pointsfile(mpss_ctx *c, const char *path) {
    return guarded([&] {
        require(c && path, "mpss_load_pointsfile: null argument");
        FILE *f = fopen(path, "rb");
        if (!f) throw Error(MPSS_ERR_INVALID, std::string("mpss_load_pointsfile: cannot open ") + path);
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        std::vector<SurfacePoint> pts((size_t)(size > 0 ? size : 0) / sizeof(SurfacePoint));
        const size_t got = pts.empty() ? 0 : fread(pts.data(), sizeof(SurfacePoint), pts.size(), f);
        fclose(f);
        if (got != pts.size()) throw Error(MPSS_ERR_INVALID, "mpss_load_pointsfile: short read");
        reinterpret_cast<Context *>(c)->set_surface_points((uint32_t)pts.size(), pts.data());
    });
}

int mpss_save_pointsfile(mpss_ctx *c, const char *path) {
    return guarded([&] {
        require(c && path, "mpss_save_pointsfile: null argument");
        const auto v = reinterpret_cast<Context *>(c)->surface_points();
        FILE *f = fopen(path, "wb");
        if (!f) throw Error(MPSS_ERR_INVALID, std::string("mpss_save_pointsfile: cannot open ") + path);
        const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(SurfacePoint), v.size(), f);
        fclose(f);
        if (put != v.size()) throw Error(MPSS_ERR_INVALID, "mpss_save_pointsfile: short write");
    });
}

int mpss_replay_samples(mpss_ctx *c, int spp, float *out, uint64_t *n_floats, int *k) {
    return guarded([&] {
        require(c && n_floats && k, "mpss_replay_samples: null argument");
        require(spp >= 1 && spp <= 32768, "mpss_replay_samples: spp out of range");
        reinterpret_cast<Context *>(c)->replay_samples(spp, out, n_floats, k);
    });
}

int mpss_get_irradiance(mpss_ctx *c, float *E, uint32_t *n) {
    return guarded([&] {
        require(c && n, "mpss_get_irradiance: null argument");
        const auto v = reinterpret_cast<Context *>(c)->irradiance();
        *n = (uint32_t)(v.size() / NB);
        if (E) memcpy(E, v.data(), sizeof(float) * v.size());
    });
}

int mpss_get_render_stats(mpss_ctx *c, mpss_render_stats *out) {
    return guarded([&] {
        require(c && out, "mpss_get_render_stats: null argument");
        *out = reinterpret_cast<Context *>(c)->render_stats();
    });
}

int mpss_set_instrumentation(mpss_ctx *c, int timing, int counting) {
    return guarded([&] {
        require(c, "mpss_set_instrumentation: null ctx");
        reinterpret_cast<Context *>(c)->set_instrumentation(timing != 0, counting);
    });
}

int mpss_set_grid_builder(mpss_ctx *c, int on_host) {
    return guarded([&] {
        require(c, "mpss_set_grid_builder: null ctx");
        reinterpret_cast<Context *>(c)->set_grid_builder(on_host != 0);
    });
}

int mpss_reset_render_stats(mpss_ctx *c) {
    return guarded([&] {
        require(c, "mpss_reset_render_stats: null ctx");
        reinterpret_cast<Context *>(c)->reset_render_stats();
    });
}

int mpss_preprocess(mpss_ctx *c, uint32_t seed) {
    return guarded([&] {
        require(c, "mpss_preprocess: null ctx");
        reinterpret_cast<Context *>(c)->preprocess(seed);
    });
}

int mpss_render_tile(mpss_ctx *c, int spp, uint32_t seed, int x0, int x1, int y0, int y1, float *out, void *stream) {
    return guarded([&] {
        require(c && out, "mpss_render_tile: null argument");
        const int32_t r[4] = {x0, x1, y0, y1};
        float *o[1] = {out};
        reinterpret_cast<Context *>(c)->render_tiles(spp, seed, 1, r, o, (hipStream_t)stream);
    });
}

int mpss_tile_costs(mpss_ctx *c, int n, const int32_t *rects, int64_t *sss_hits, int64_t *surf_hits) {
    return guarded([&] {
        require(c && n >= 0 && (n == 0 || (rects && sss_hits && surf_hits)), "mpss_tile_costs: null argument");
        reinterpret_cast<Context *>(c)->tile_costs(n, rects, sss_hits, surf_hits);
    });
}

int mpss_render_tiles(mpss_ctx *c, int spp, uint32_t seed, int n, const int32_t *rects, float *const *outs,
                      void *stream) {
    return guarded([&] {
        require(c && n >= 0 && (n == 0 || (rects && outs)), "mpss_render_tiles: null argument");
        reinterpret_cast<Context *>(c)->render_tiles(spp, seed, n, rects, outs, (hipStream_t)stream);
    });
}

}  // extern "C"

// ---------------------------------------------------------------- host-side utilities
extern "C" {

int mpss_mc_profile(mpss_ctx *c, const mpss_layer *layers, int n, float mfp_range, int nseg, uint64_t nphotons,
                    uint64_t seed, double *refl, double *trans, double *tr, double *tt, uint64_t *events,
                    void *stream) {
    return guarded([&] {
        require(c && layers && refl && trans && tr && tt, "mpss_mc_profile: null argument");
        Context &ctx = *reinterpret_cast<Context *>(c);
        MPSS_HIP(hipSetDevice(ctx.config().device));
        static_assert(sizeof(mpss_layer) == sizeof(McLayer), "layer layout");
        const McScene sc = make_mc_scene(reinterpret_cast<const McLayer *>(layers), n, (double)mfp_range, nseg);
        run_mc_profile(sc, nphotons, seed, refl, trans, tr, tt, events, (hipStream_t)stream);
    });
}

int mpss_mc_reference(const mpss_layer *layers, int n, float mfp_range, int nseg, int lerp, double *refl,
                      double *trans, double *tr, double *tt) {
    return guarded([&] {
        require(layers && refl && trans && tr && tt, "mpss_mc_reference: null argument");
        require(n >= 1 && n <= 8 && nseg >= 1 && nseg <= (1 << 16), "mpss_mc_reference: bad layer or ring count");
        std::vector<MpcLayer> ml(n);
        double mfp_total = 0.;
        for (int i = 0; i < n; ++i) {
            require(layers[i].musp > 0.f && layers[i].mua >= 0.f && layers[i].thickness > 0.f,
                    "mpss_mc_reference: layers need musp > 0, mua >= 0, thickness > 0");
            ml[i] = MpcLayer{layers[i].mua, layers[i].musp, layers[i].ior, layers[i].thickness};
            mfp_total += 1. / (double)(layers[i].mua + layers[i].musp);  // Render, mcprofile.cpp:457-463
        }
        const double extent = mfp_range * (mfp_total / (double)n);
        mc_reference_profile(ml.data(), n, extent, nseg, lerp != 0, refl, trans, tr, tt);
    });
}

int mpss_mc_profile_batch(mpss_ctx *c, const mpss_layer *layers, int nslabs, int n, float mfp_range, int nseg,
                          uint64_t nphotons, uint64_t seed, double *refl, double *trans, double *tr, double *tt,
                          uint64_t *events, void *stream) {
    return guarded([&] {
        require(c && layers && tr && tt, "mpss_mc_profile_batch: null argument");
        require(nslabs >= 1 && nslabs <= kMcMaxSlabs, "mpss_mc_profile_batch: 1..65536 slabs supported");
        // every slab is validated (as mpss_mc_profile validates its one) before the device is touched
        std::vector<McScene> sc((size_t)nslabs);
        for (int s = 0; s < nslabs; ++s)
            sc[s] = make_mc_scene(reinterpret_cast<const McLayer *>(layers) + (size_t)s * std::max(n, 0), n,
                                  (double)mfp_range, nseg);
        Context &ctx = *reinterpret_cast<Context *>(c);
        MPSS_HIP(hipSetDevice(ctx.config().device));
        run_mc_profile_batch(sc.data(), nslabs, nphotons, seed, refl, trans, tr, tt, events, (hipStream_t)stream);
    });
}

int mpss_mc_reference_batch(mpss_ctx *c, const mpss_layer *layers, int nslabs, int n, float mfp_range, int nseg,
                            int desired_length, int lerp, int max_batch, double *refl, double *trans, double *tr,
                            double *tt, void *stream) {
    return guarded([&] {
        require(c && layers && tr && tt, "mpss_mc_reference_batch: null argument");
        require(nslabs >= 1 && nslabs <= kMcMaxSlabs, "mpss_mc_reference_batch: 1..65536 slabs supported");
        require(n >= 1 && n <= 8 && nseg >= 1 && nseg <= (1 << 16), "mpss_mc_reference_batch: bad layer or ring count");
        require(desired_length >= 2 && desired_length <= 1024, "mpss_mc_reference_batch: desired length outside 2..1024");
        std::vector<MpcLayer> ml((size_t)nslabs * n);
        std::vector<double> extent((size_t)nslabs);
        for (int s = 0; s < nslabs; ++s) {
            double mfp_total = 0.;
            for (int i = 0; i < n; ++i) {
                const mpss_layer &l = layers[(size_t)s * n + i];
                require(l.musp > 0.f && l.mua >= 0.f && l.thickness > 0.f,
                        "mpss_mc_reference_batch: layers need musp > 0, mua >= 0, thickness > 0");
                ml[(size_t)s * n + i] = MpcLayer{l.mua, l.musp, l.ior, l.thickness};
                mfp_total += 1. / (double)(l.mua + l.musp);  // Render, mcprofile.cpp:457-463
            }
            extent[s] = mfp_range * (mfp_total / (double)n);
        }
        if (n != 2) {  // the GPU builder combines two layers; other stacks take the host path, slab by slab
            std::vector<double> r((size_t)nseg), t((size_t)nseg);
            for (int s = 0; s < nslabs; ++s) {
                mc_reference_profile(&ml[(size_t)s * n], n, extent[s], nseg, lerp != 0, r.data(), t.data(), tr + s,
                                     tt + s, desired_length);
                if (refl) std::copy(r.begin(), r.end(), refl + (size_t)s * nseg);
                if (trans) std::copy(t.begin(), t.end(), trans + (size_t)s * nseg);
            }
            return;
        }
        Context &ctx = *reinterpret_cast<Context *>(c);
        MPSS_HIP(hipSetDevice(ctx.config().device));
        mc_reference_batch_gpu(ml.data(), nslabs, extent.data(), nseg, desired_length, lerp != 0, max_batch, refl,
                               trans, tr, tt, (hipStream_t)stream);
    });
}

int mpss_host_tessellate(uint32_t nv, const float *P, const float *N, const float *S, const float *uv, uint32_t nt,
                         const int32_t *idx, const float *o2w, const float *w2o, int flip, uint32_t mat,
                         float min_dist, int incenter, void *rec, uint32_t *n) {
    return mpss_host_tessellate_bumped(nv, P, N, S, uv, nt, idx, o2w, w2o, flip, mat, min_dist, incenter, nullptr, rec,
                                       n);
}

int mpss_host_imagemap_lookup(const mpss_imagemap *t, uint32_t n, const float *uvd, float *out) {
    return guarded([&] {
        require(t && (n == 0 || (uvd && out)), "mpss_host_imagemap_lookup: null argument");
        const std::unique_ptr<ImageTexture> tex = build_imagemap(*t);
        for (uint32_t i = 0; i < n; ++i) {
            const float *a = uvd + 6 * (size_t)i;
            const UVDiff g{a[0], a[1], a[2], a[3], a[4], a[5]};
            tex_eval(tex->host, g, out + 3 * (size_t)i);
        }
    });
}

int mpss_host_tessellate_bumped(uint32_t nv, const float *P, const float *N, const float *S, const float *uv,
                                uint32_t nt, const int32_t *idx, const float *o2w, const float *w2o, int flip,
                                uint32_t mat, float min_dist, int incenter, const mpss_imagemap *bump, void *rec,
                                uint32_t *n) {
    return guarded([&] {
        require(P && idx && o2w && w2o && n && nv > 0 && min_dist > 0.f, "mpss_host_tessellate: bad argument");
        SceneData sd;
        Mesh m;
        m.P.assign(P, P + 3 * (size_t)nv);
        if (N) m.N.assign(N, N + 3 * (size_t)nv);
        if (S) m.S.assign(S, S + 3 * (size_t)nv);
        if (uv) m.uv.assign(uv, uv + 2 * (size_t)nv);
        m.idx.assign(idx, idx + 3 * (size_t)nt);
        for (int32_t v : m.idx) require(v >= 0 && (uint32_t)v < nv, "mpss_host_tessellate: index out of range");
        memcpy(m.o2w, o2w, sizeof(m.o2w));
        memcpy(m.w2o, w2o, sizeof(m.w2o));
        m.reverse_orientation = flip != 0;
        m.swaps_handedness = false;
        m.material = mat;
        sd.meshes.push_back(std::move(m));
        std::vector<SurfacePoint> pts;
        std::unique_ptr<ImageTexture> bt;
        std::vector<const TexView *> bv;
        if (bump) {
            require(bump->is_float != 0, "mpss_host_tessellate_bumped: the bumpmap is a float texture");
            bt = build_imagemap(*bump);
            bv.assign((size_t)mat + 1, nullptr);
            bv[mat] = &bt->host;
        }
        tessellate_surface_points(sd, min_dist, incenter != 0, pts, 0, bump ? bv.data() : nullptr);
        if (rec) {
            require(*n >= pts.size(), "mpss_host_tessellate: records buffer too small");
            memcpy(rec, pts.data(), pts.size() * sizeof(SurfacePoint));
        }
        *n = (uint32_t)pts.size();
    });
}

int mpss_host_from_rgb(const float *rgb, int illuminant, float *out) {
    return guarded([&] {
        require(rgb && out, "mpss_host_from_rgb: null argument");
        spectrum_from_rgb(rgb, illuminant != 0, out);
    });
}

int mpss_host_skin_layers(const mpss_layeredskin *m, float *mua, float *musp, float *thickness, float *eta) {
    return guarded([&] {
        require(m && mua && musp && thickness && eta, "mpss_host_skin_layers: null argument");
        SkinParams sp;
        sp.roughness = m->roughness;
        sp.nmperunit = m->nmperunit;
        sp.f_mel = m->f_mel;
        sp.f_eu = m->f_eu;
        sp.f_blood = m->f_blood;
        sp.f_ohg = m->f_ohg;
        for (int l = 0; l < 2; ++l) {
            sp.thickness_nm[l] = m->layer_thickness_nm[l];
            sp.ior[l] = m->layer_ior[l];
        }
        LayerParams lp;
        skin_layer_params(sp, lp);
        memcpy(mua, lp.mua, sizeof(lp.mua));
        memcpy(musp, lp.musp, sizeof(lp.musp));
        memcpy(thickness, lp.thickness, sizeof(lp.thickness));
        memcpy(eta, lp.eta, sizeof(lp.eta));
    });
}

int mpss_host_build_profile(const float *mua, const float *musp, const float *thickness, const float *eta,
                            int desired_length, int lerp, float *rd, uint32_t *length, float *rcp, float *total) {
    return guarded([&] {
        require(mua && musp && thickness && eta && length, "mpss_host_build_profile: null argument");
        require(desired_length >= 2 && desired_length <= 4096, "desired_length out of range");
        LayerParams lp;
        memcpy(lp.mua, mua, sizeof(lp.mua));
        memcpy(lp.musp, musp, sizeof(lp.musp));
        memcpy(lp.thickness, thickness, sizeof(lp.thickness));
        memcpy(lp.eta, eta, sizeof(lp.eta));
        ProfileTables pt;
        build_profile(lp, desired_length, lerp != 0, pt);
        *length = (uint32_t)pt.length;
        if (rd) memcpy(rd, pt.table.data(), sizeof(float) * pt.table.size());
        if (rcp) memcpy(rcp, pt.rcp, sizeof(pt.rcp));
        if (total) memcpy(total, pt.total_reflectance, sizeof(pt.total_reflectance));
    });
}

int mpss_host_dipole_rd(const float *sigma_a, const float *sigmap_s, float eta, uint32_t n, const float *d2, float *rd,
                        float *total) {
    return guarded([&] {
        require(sigma_a && sigmap_s && (n == 0 || (d2 && rd)), "mpss_host_dipole_rd: null argument");
        DipoleRd d;
        dipole_init(sigma_a, sigmap_s, eta, d);
        for (uint32_t i = 0; i < n; ++i) dipole_eval(d, d2[i], rd + (size_t)i * NB);
        if (total) dipole_total(d, total);
    });
}

int mpss_host_rho_table(float roughness, float eta, int fixed, int n, int sq, float *hd, float *hh) {
    return guarded([&] {
        require(hd && n >= 2 && sq >= 1, "mpss_host_rho_table: bad argument");
        RhoTable rt;
        build_rho_table(roughness, eta, fixed != 0, n, sq, rt);
        memcpy(hd, rt.hd.data(), sizeof(float) * n);
        if (hh) *hh = rt.hh;
    });
}

int mpss_host_octree_export(uint32_t n, const float *p, const float *nrm, const float *E, const float *area,
                            uint32_t *n_nodes, float *node_p, float *node_area, float *node_et, int32_t *depth,
                            int32_t *skip, int32_t *leaf_first, int32_t *leaf_count, int32_t *order) {
    return guarded([&] {
        require(p && nrm && E && area && n_nodes && n > 0, "mpss_host_octree_export: bad argument");
        FlatOctree t;
        build_octree((int)n, p, nrm, E, area, t);
        *n_nodes = (uint32_t)t.hdr.size();
        for (size_t i = 0; i < t.hdr.size(); ++i) {
            const NodeHdr &h = t.hdr[i];
            if (node_p) { node_p[3 * i] = h.px; node_p[3 * i + 1] = h.py; node_p[3 * i + 2] = h.pz; }
            if (node_area) node_area[i] = h.sum_area;
            if (node_et) memcpy(node_et + i * NB, &t.node_et[i * ROW], sizeof(float) * NB);
            if (depth) depth[i] = h.depth;
            if (skip) skip[i] = h.skip;
            if (leaf_first) leaf_first[i] = h.leaf_first;
            if (leaf_count) leaf_count[i] = h.leaf_count;
        }
        if (order) memcpy(order, t.pt_index.data(), sizeof(int32_t) * t.pt_index.size());
    });
}

void mpss_profilefit_defaults(mpss_profilefit *f) {
    if (!f) return;
    memset(f, 0, sizeof(*f));
    f->layer_thickness_nm[0] = 0.25e6f;  // the fork's default layers (layeredskin.cpp:250-253)
    f->layer_thickness_nm[1] = 20e6f;
    f->layer_ior[0] = f->layer_ior[1] = 1.4f;
    f->desired_length = 256;
    f->id_min = 0;
    f->id_max = -1;
    f->max_profiles_per_batch = 0;
}

int mpss_profilefit_params(const mpss_profilefit *f, uint32_t id, float *out) {
    return guarded([&] {
        require(f && out, "mpss_profilefit_params: null argument");
        const FitPlan pl = make_fit_plan(*f, false);
        require(id < pl.total, "mpss_profilefit_params: id out of range");
        pl.params(id, out);
    });
}

int mpss_profilefit_layers(const mpss_profilefit *f, uint32_t id, float *mua, float *musp, float *thickness,
                           float *eta) {
    return guarded([&] {
        require(f && mua && musp && thickness && eta, "mpss_profilefit_layers: null argument");
        const FitPlan pl = make_fit_plan(*f, false);
        require(id < pl.total, "mpss_profilefit_layers: id out of range");
        float v[4];
        pl.params(id, v);
        LayerParams lp;
        skin_fit_layer_params(v[0], v[1], v[2], v[3], f->layer_thickness_nm, f->layer_ior, lp);
        memcpy(mua, lp.mua, sizeof(lp.mua));
        memcpy(musp, lp.musp, sizeof(lp.musp));
        memcpy(thickness, lp.thickness, sizeof(lp.thickness));
        memcpy(eta, lp.eta, sizeof(lp.eta));
    });
}

int mpss_host_sog_solve(const double *a, const double *b, int quirk, double *x) {
    return guarded([&] {
        require(a && b && x, "mpss_host_sog_solve: null argument");
        sog_solve6(a, b, x, quirk != 0);
    });
}

int mpss_host_sog_fit(uint32_t n, uint32_t length, const float *dist_sq, const float *data, uint32_t n_sigmas,
                      const float *sigmas, const float *mfp_min, const float *mfp_max, float *coeffs, float *error,
                      int32_t *centre, float *cand_error, float *cand_coeffs, double *cand_gram) {
    return guarded([&] {
        require(dist_sq && data && sigmas && mfp_min && mfp_max && coeffs && error && centre,
                "mpss_host_sog_fit: null argument");
        require(length >= 1 && n_sigmas >= 6 && n_sigmas <= 4096, "mpss_host_sog_fit: needs samples and 6 .. 4096 sigmas");
        const int64_t bad = sog_fit_host(n, length, dist_sq, data, (int)n_sigmas, sigmas, mfp_min, mfp_max, coeffs,
                                         error, centre, cand_error, cand_coeffs, cand_gram);
        if (bad >= 0)
            throw Error(MPSS_ERR_INTERNAL, "mpss_host_sog_fit: profile " + std::to_string(bad) +
                                               " has no candidate window");
    });
}

int mpss_sog_fit(mpss_ctx *c, uint32_t n, uint32_t length, const float *dist_sq, const float *data, uint32_t n_sigmas,
                 const float *sigmas, const float *mfp_min, const float *mfp_max, float *coeffs, float *error,
                 int32_t *centre, float *cand_error, float *cand_coeffs, void *stream) {
    return guarded([&] {
        require(c && dist_sq && data && sigmas && mfp_min && mfp_max && coeffs && error && centre,
                "mpss_sog_fit: null argument");
        require(n >= 1 && length >= 1 && n_sigmas >= 6 && n_sigmas <= 4096,
                "mpss_sog_fit: needs profiles, samples and 6 .. 4096 sigmas");
        Context &ctx = *reinterpret_cast<Context *>(c);
        auto lock = ctx.lock_device();
        hipStream_t st = (hipStream_t)stream;
        const size_t cells = (size_t)n * length;
        DevBuf<float> d_d, d_y, d_coeffs, d_err;
        DevBuf<int32_t> d_centre;
        d_d.upload(dist_sq, cells);
        d_y.upload(data, cells);
        d_coeffs.alloc((size_t)n * n_sigmas);
        d_err.alloc(n);
        d_centre.alloc(n);
        SogFitWork w;
        sog_fit_prepare(n, n, (int)n_sigmas, sigmas, mfp_min, mfp_max, w);
        sog_fit_launch(0, n, length, d_d.ptr, d_y.ptr, d_coeffs.ptr, d_err.ptr, d_centre.ptr, w, st);
        MPSS_HIP(hipMemcpyAsync(coeffs, d_coeffs.ptr, sizeof(float) * n * n_sigmas, hipMemcpyDeviceToHost, st));
        MPSS_HIP(hipMemcpyAsync(error, d_err.ptr, sizeof(float) * n, hipMemcpyDeviceToHost, st));
        MPSS_HIP(hipMemcpyAsync(centre, d_centre.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        if (cand_error)
            MPSS_HIP(hipMemcpyAsync(cand_error, w.cand_error.ptr, sizeof(float) * n * n_sigmas, hipMemcpyDeviceToHost, st));
        if (cand_coeffs)
            MPSS_HIP(hipMemcpyAsync(cand_coeffs, w.cand_coeffs.ptr, sizeof(float) * n * n_sigmas * 6,
                                    hipMemcpyDeviceToHost, st));
        MPSS_HIP(hipStreamSynchronize(st));
        for (uint32_t p = 0; p < n; ++p)
            if (centre[p] < 0)
                throw Error(MPSS_ERR_INTERNAL, "mpss_sog_fit: profile " + std::to_string(p) + " has no candidate window");
    });
}

int mpss_profile_fit(mpss_ctx *c, const mpss_profilefit *f, uint32_t *n_sigmas, uint32_t *n_ids, float *sigmas,
                     float *coeffs, float *error, float *rgb, int32_t *centre, double *stage_ms, void *stream) {
    return guarded([&] {
        require(c && f && n_sigmas && n_ids, "mpss_profile_fit: null argument");
        const FitPlan pl = make_fit_plan(*f);
        const uint32_t ns = (uint32_t)pl.sigmas.size(), ni = pl.id1 - pl.id0;
        *n_sigmas = ns;
        *n_ids = ni;
        if (sigmas) memcpy(sigmas, pl.sigmas.data(), sizeof(float) * ns);
        if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = 0.;
        if (!coeffs || ni == 0) return;
        std::vector<LayerParams> lp;
        std::vector<float> mfp_min, mfp_max;
        fit_layers(*f, pl, lp, mfp_min, mfp_max);
        const uint32_t P = ni * NB;
        // a band without a candidate is known before anything is launched
        require(ns >= 6, "mpss_profile_fit: the grid's mfp range gives fewer than 6 sigmas");
        for (uint32_t p = 0; p < P; ++p) {
            int first, count;
            sog_candidates((int)ns, pl.sigmas.data(), mfp_min[p], mfp_max[p], first, count);
            if (!count) fit_no_candidate(pl, p);
        }
        Context &ctx = *reinterpret_cast<Context *>(c);
        auto lock = ctx.lock_device();
        hipStream_t st = (hipStream_t)stream;
        const int nent = fit_profile_samples(f->desired_length);
        // Every allocation and host copy of both stages happens here, before anything is queued: from the
        // first batch's memset to the copy back, the host only queues work on `st`.
        FitProfileWork pw;
        SogFitWork fw;
        const uint32_t batch = (uint32_t)fit_profiles_prepare(lp.data(), (int)P, f->desired_length,
                                                              f->max_profiles_per_batch, pw);
        sog_fit_prepare(P, batch, (int)ns, pl.sigmas.data(), mfp_min.data(), mfp_max.data(), fw);
        const uint32_t nbatch = (P + batch - 1) / batch;
        DevBuf<float> d_d, d_y, d_coeffs, d_err;  // d^2 and R of one batch; the results of all P
        DevBuf<int32_t> d_centre;
        d_d.alloc((size_t)batch * nent);
        d_y.alloc((size_t)batch * nent);
        d_coeffs.alloc((size_t)P * ns);
        d_err.alloc(P);
        d_centre.alloc(P);
        struct Events {
            std::vector<hipEvent_t> e;
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) (void)hipEventDestroy(x);
            }
        } ev;
        if (stage_ms) {
            ev.e.assign((size_t)3 * nbatch, nullptr);
            for (hipEvent_t &x : ev.e) MPSS_HIP(hipEventCreate(&x));
        }
        for (uint32_t b = 0; b < nbatch; ++b) {
            const uint32_t c0 = b * batch, nch = std::min(batch, P - c0);
            if (stage_ms) MPSS_HIP(hipEventRecord(ev.e[3 * b], st));
            fit_profiles_launch((int)c0, (int)nch, d_d.ptr, d_y.ptr, pw, st);
            if (stage_ms) MPSS_HIP(hipEventRecord(ev.e[3 * b + 1], st));
            // the fit reads the batch's d^2 and R where the profile stage left them: no wait, no copy
            sog_fit_launch(c0, nch, (uint32_t)nent, d_d.ptr, d_y.ptr, d_coeffs.ptr + (size_t)c0 * ns, d_err.ptr + c0,
                           d_centre.ptr + c0, fw, st);
            if (stage_ms) MPSS_HIP(hipEventRecord(ev.e[3 * b + 2], st));
        }
        std::vector<float> err(P);
        std::vector<int32_t> cen(P);
        MPSS_HIP(hipMemcpyAsync(coeffs, d_coeffs.ptr, sizeof(float) * (size_t)P * ns, hipMemcpyDeviceToHost, st));
        MPSS_HIP(hipMemcpyAsync(err.data(), d_err.ptr, sizeof(float) * P, hipMemcpyDeviceToHost, st));
        MPSS_HIP(hipMemcpyAsync(cen.data(), d_centre.ptr, sizeof(int32_t) * P, hipMemcpyDeviceToHost, st));
        MPSS_HIP(hipStreamSynchronize(st));
        if (stage_ms) {
            for (uint32_t b = 0; b < nbatch; ++b) {
                float ms = 0.f;
                MPSS_HIP(hipEventElapsedTime(&ms, ev.e[3 * b], ev.e[3 * b + 1]));
                stage_ms[0] += ms;
                MPSS_HIP(hipEventElapsedTime(&ms, ev.e[3 * b + 1], ev.e[3 * b + 2]));
                stage_ms[1] += ms;
            }
            stage_ms[2] = (double)pw.batches;
        }
        if (error) memcpy(error, err.data(), sizeof(float) * P);
        if (centre) memcpy(centre, cen.data(), sizeof(int32_t) * P);
        for (uint32_t p = 0; p < P; ++p)
            if (cen[p] < 0) fit_no_candidate(pl, p);  // (every candidate's error was NaN)
        if (rgb) fit_rgb_rows(ni, ns, coeffs, rgb);
    });
}

int mpss_host_profile_fit(const mpss_profilefit *f, uint32_t *n_sigmas, uint32_t *n_ids, float *sigmas, float *coeffs,
                          float *error, float *rgb, int32_t *centre, uint32_t *length, float *pd, float *py) {
    return guarded([&] {
        require(f && n_sigmas && n_ids, "mpss_host_profile_fit: null argument");
        const FitPlan pl = make_fit_plan(*f);
        const uint32_t ns = (uint32_t)pl.sigmas.size(), ni = pl.id1 - pl.id0;
        *n_sigmas = ns;
        *n_ids = ni;
        if (sigmas) memcpy(sigmas, pl.sigmas.data(), sizeof(float) * ns);
        if (length) *length = 0;
        if (!coeffs || ni == 0) return;
        std::vector<LayerParams> lp;
        std::vector<float> mfp_min, mfp_max;
        fit_layers(*f, pl, lp, mfp_min, mfp_max);
        require(ns >= 6, "mpss_host_profile_fit: the grid's mfp range gives fewer than 6 sigmas");
        const uint32_t P = ni * NB;
        const size_t L0 = (size_t)fit_profile_samples_host(f->desired_length);
        std::vector<float> dd((size_t)P * L0), yy((size_t)P * L0);
        {  // one profile per task over a few host threads (each profile is its own FFTs)
            std::atomic<uint32_t> next{0};
            std::atomic<bool> failed{false};
            std::vector<std::thread> th;
            const unsigned nt = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), P}));
            for (unsigned t = 0; t < nt; ++t)
                th.emplace_back([&] {
                    std::vector<float> d, y;
                    for (uint32_t p; (p = next.fetch_add(1)) < P;) {
                        try {
                            fit_channel_profile(lp[p / NB], (int)(p % NB), f->desired_length, d, y);
                            if (d.size() != L0) throw Error(MPSS_ERR_INTERNAL, "profile length");
                            memcpy(&dd[(size_t)p * L0], d.data(), sizeof(float) * L0);
                            memcpy(&yy[(size_t)p * L0], y.data(), sizeof(float) * L0);
                        } catch (...) {
                            failed = true;
                        }
                    }
                });
            for (auto &x : th) x.join();
            if (failed) throw Error(MPSS_ERR_INTERNAL, "mpss_host_profile_fit: a host profile build failed");
        }
        const uint32_t L = (uint32_t)(dd.size() / P);
        if (length) *length = L;
        if (pd) memcpy(pd, dd.data(), sizeof(float) * dd.size());
        if (py) memcpy(py, yy.data(), sizeof(float) * yy.size());
        std::vector<float> err(P);
        std::vector<int32_t> cen(P);
        const int64_t bad = sog_fit_host(P, L, dd.data(), yy.data(), (int)ns, pl.sigmas.data(), mfp_min.data(),
                                         mfp_max.data(), coeffs, err.data(), cen.data(), nullptr, nullptr, nullptr);
        if (error) memcpy(error, err.data(), sizeof(float) * P);
        if (centre) memcpy(centre, cen.data(), sizeof(int32_t) * P);
        if (bad >= 0) fit_no_candidate(pl, bad);
        if (rgb) fit_rgb_rows(ni, ns, coeffs, rgb);
    });
}

}  // extern "C"
