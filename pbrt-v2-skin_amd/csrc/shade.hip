// shade.hip -- direct lighting of the compacted hits, step 2 of a render batch (DESIGN.md "A render
// batch"), between primary_kernel and the Mo() gather:
//   shade_tex_kernel       GetBSDF's albedo / bump lookups with ray differentials (layeredskin.cpp:143-185)
//   shade_direct_kernel    one EstimateDirect per lane (core/integrator.cpp:117-174)
//   shade_nolight_kernel   a scene without lights
//   direct_combine_kernel  UniformSampleAllLights' per-band sums (integrator.cpp:47-77)
// and their *_spec_kernel instances for a scene with Kr / Kt textures (RenderScene::any_spec_tex), where a
// hit's R, T and lobe set come from its own lookups (HitSpec); every other scene runs the kernels above.
#include "render.h"

#include <climits>
#include <type_traits>

#include "bvh_trace.h"
#include "geom.h"
#include "light_sample.h"
#include "pixel_sample.h"
#include "spectrum_tables.h"

namespace mpss {

// One lobe value of the layer-0 BSDF for a direction pair (BSDF::f, reflection.cpp:765-779):
// kind 1 = Microfacet (R * D * G * F / den), kind 2 = MicrofacetTransmission (T * s * (1 - F)).
// The transmission lobe and the infinite light run only for the materials / scenes that have
// them; they are called out of line so the common path keeps its code small (I-cache).
__device__ __noinline__ MtTerms mt_terms_ool(const Microfacet &m, V3 wo, V3 wi) { return mt_terms(m, wo, wi); }
__device__ __noinline__ float mt_pdf_ool(const Microfacet &m, V3 wo, V3 wi) { return mt_pdf(m, wo, wi); }
__device__ __noinline__ void mt_sample_ool(const Microfacet &m, V3 wo, float u1, float u2, V3 &wi, float &pdf) {
    mt_sample(m, wo, u1, u2, wi, pdf);
}

struct Lobe {
    uint32_t kind;
    float a, b, c, d;
};

// What GetBSDF makes of Kr and Kt at a mesh hit (layeredskin.cpp:154-161): R, T, and which of the two
// lobes exist (!R.IsBlack(), !T.IsBlack()). MatSpec: constant Kr / Kt, the material's record. HitSpec: a
// scene with Kr / Kt textures -- a textured side is FromRGB of the hit's lookup (ImageTexture's
// convertOut; hit_kr / hit_kt, whose w is that spectrum's blackness test), the other side the material's.
struct MatSpec {
    const RenderMaterial *mat;
    __device__ __forceinline__ int has_refl() const { return mat->has_refl; }
    __device__ __forceinline__ int has_trans() const { return mat->has_trans; }
    __device__ __forceinline__ float R(int c) const { return mat->R[c]; }
    __device__ __forceinline__ float T(int c) const { return mat->T[c]; }
};
struct HitSpec {
    const RenderMaterial *mat;
    int refl, trans;
    bool r_tex, t_tex;
    ReflSplit r, t;
    __device__ __forceinline__ int has_refl() const { return refl; }
    __device__ __forceinline__ int has_trans() const { return trans; }
    __device__ __forceinline__ float R(int c) const { return r_tex ? refl_split_band(r, c) : mat->R[c]; }
    __device__ __forceinline__ float T(int c) const { return t_tex ? refl_split_band(t, c) : mat->T[c]; }
};
template <bool kSpec>
using SpecOf = std::conditional_t<kSpec, HitSpec, MatSpec>;
__device__ __forceinline__ void load_spec(MatSpec &b, const RenderMaterial *mat, const SampleRecs &, int) { b.mat = mat; }
__device__ __forceinline__ void load_spec(HitSpec &b, const RenderMaterial *mat, const SampleRecs &rec, int slot) {
    b = HitSpec{};
    b.mat = mat;
    if (!mat) return;  // a light sphere's surface
    b.refl = mat->has_refl;
    b.trans = mat->has_trans;
    if (mat->has_kr_tex) {
        const float4 k = rec.hit_kr[slot];
        b.r_tex = true;
        b.r = refl_split(k.x, k.y, k.z);
        b.refl = k.w != 0.f;
    }
    if (mat->has_kt_tex) {
        const float4 k = rec.hit_kt[slot];
        b.t_tex = true;
        b.t = refl_split(k.x, k.y, k.z);
        b.trans = k.w != 0.f;
    }
}

// The shading point's BSDF is a mesh material's (b.mat, with the hit's R / T / lobe set b), or -- b.mat ==
// nullptr -- the default matte of a light sphere seen directly (geom.h kMatteF): kind 3, f = 0 + R * INV_PI
// on the reflection side.
template <class B>
__device__ __forceinline__ Lobe bsdf_lobe(const B &b, bool refl, V3 wo_l, V3 wi_l) {
    Lobe L{0u, 0.f, 0.f, 0.f, 1.f};
    if (!b.mat) {
        if (refl) L = Lobe{3u, 0.f + kMatteF, 0.f, 0.f, 1.f};
    } else if (refl) {  // the ng test keeps BRDFs only
        if (b.has_refl()) {
            const MfTerms t = microfacet_terms(b.mat->mf, wo_l, wi_l);
            if (!t.zero) L = Lobe{1u, t.D, t.G, t.F, t.den};
        }
    } else if (b.has_trans()) {  // ... or BTDFs only
        const MtTerms t = mt_terms_ool(b.mat->mf, wo_l, wi_l);
        if (!t.zero) L = Lobe{2u, t.s, t.F, 0.f, 1.f};
    }
    return L;
}

template <class B>
__device__ __forceinline__ float lobe_value(const B &b, const Lobe &L, int c) {
    if (L.kind == 3u) return L.a;
    return L.kind == 1u ? b.R(c) * L.a * L.b * L.c / L.d : (b.T(c) * L.a) * (1.f - L.b);
}

// x / d (IEEE, correctly rounded) for many x over one d, from inv = x-independent RN(1 / d): with
// q = RN(x inv) and the exact residual r = x - d q (one FMA), RN(q + r inv) is RN(x / d) -- Markstein's
// correction, valid when nothing under- or overflows (it replaces the ~10-instruction IEEE division
// sequence by 3 instructions; tools/check_div.c runs it against x / d on 2e8 random operand pairs, 0
// differences). Outside the guarded range, and when d itself is out of range (dok false), it divides.
__device__ __forceinline__ float div_by(float x, float d, float inv, bool dok) {
    const float q = x * inv;
    const float r = __builtin_fmaf(-d, q, x);
    const float q1 = __builtin_fmaf(r, inv, q);
    const float ax = fabsf(x), aq = fabsf(q1);
    if (dok && ax >= 0x1p-100f && ax <= 0x1p100f && aq >= 0x1p-100f && aq <= 0x1p100f) return q1;
    return x / d;
}
struct Den {  // one denominator shared by the 30 bands
    float d, inv;
    bool ok;
};
__device__ __forceinline__ Den make_den(float d) {
    const float ad = fabsf(d);
    return Den{d, 1.f / d, ad >= 0x1p-60f && ad <= 0x1p60f};
}
// lobe_value with the reflection lobe's division by L.d done through den = make_den(L.d)
template <class B>
__device__ __forceinline__ float lobe_value_den(const B &b, const Lobe &L, int c, const Den &den) {
    if (L.kind == 3u) return L.a;
    return L.kind == 1u ? div_by(b.R(c) * L.a * L.b * L.c, den.d, den.inv, den.ok) : (b.T(c) * L.a) * (1.f - L.b);
}

template <class B>
__device__ __forceinline__ bool lobe_black(const B &b, const Lobe &L) {
    if (L.kind == 0u) return true;
    if (L.kind == 3u) return false;
    for (int c = 0; c < NB; ++c)
        if (lobe_value(b, L, c) != 0.f) return false;
    return true;
}

// BSDF::Pdf (reflection.cpp:736-751): mean of the matching lobes' pdfs, R then T
template <class B>
__device__ __forceinline__ float bsdf_pdf(const B &b, V3 wo_l, V3 wi_l) {
    if (!b.mat) return lambert_pdf(wo_l, wi_l);  // (0 + pdf) / 1
    const int n = b.has_refl() + b.has_trans();
    if (n == 0) return 0.f;
    float pdf = 0.f;
    if (b.has_refl()) pdf += microfacet_pdf(b.mat->mf, wo_l, wi_l);
    if (b.has_trans()) pdf += mt_pdf_ool(b.mat->mf, wo_l, wi_l);
    return pdf / (float)n;
}

// ------------------------------------------------------------------ shading + direct light
// The rest of MultipoleSubsurfaceIntegrator::Li for the compacted surface hits, with one lane
// per (hit, light, light-sample j) of UniformSampleAllLights (integrator.cpp:47-77): each lane
// runs one EstimateDirect (:117-174) -- light sample + shadow ray, BSDF sample + ray -- and
// stores its scalars; direct_combine_kernel then forms the per-band sums in the reference's
// order (j ascending inside a light, lights ascending). BSDF values are a 30-band factor times
// scalars (Lobe), so no lane carries a spectrum.
struct DirectTerms {       // 16 words: one EstimateDirect
    float k1, adn, w2, pdf2;   // light term f * Li * k1; BSDF term f * Li * adn * w2 / pdf2
    Lobe l1, l2;               // the BSDF lobe value of each term (kind 0: term absent)
    float pad[2];
};
static_assert(sizeof(DirectTerms) == 64, "one 64-B record per light sample");

// kSpec: the hit's R, T and lobe set from its Kr / Kt lookups (HitSpec) -- shade_direct_spec_kernel
template <bool kSpec>
__device__ __forceinline__ void shade_direct(const RenderScene &sc, const SampleRecs &rec, int spp, uint32_t seed,
                                             int max_hits, int ns_max, DirectTerms *terms,
                                             float4 *__restrict__ inf_st) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int per_hit = sc.nlights * ns_max;
    const int nhits = *rec.hit_count;
    if ((int64_t)blockIdx.x * blockDim.x >= (int64_t)nhits * per_hit) return;
    const int slot = (int)(gid / per_hit);
    if (slot >= nhits || slot >= max_hits) return;
    const int lj = (int)(gid % per_hit), l = lj / ns_max, j = lj % ns_max;
    const uint32_t hs = rec.hit_s[slot];
    const bool lsurf = (hs & HS_LSURF) != 0;  // a light sphere's own surface: matte, no Mo()
    if ((hs & HS_LIGHT) && !lsurf) {  // a miss with infinite lights: no shading point, no Mo()
        if (lj == 0) rec.hit_q[slot] = make_float4(0.f, 0.f, 0.f, -1.f);
        return;
    }
    const RenderLight &L = sc.lights[l];
    const int ns = L.nsamples_round;
    DirectTerms out{};
    if (j >= ns && lj != 0) return;
    const float4 ha = rec.hit_a[slot], hb = rec.hit_b[slot];
    const int s = (int)(hs & 0xffffu);
    const uint32_t mid = (hs >> REC_MAT_SHIFT) & 0xffu;
    const bool sss = (hs >> 31) != 0;
    const int tri = __float_as_int(ha.w);
    const uint32_t pix = __float_as_uint(hb.w);
    const V3 d = V3{hb.x, hb.y, hb.z};
    const V3 o = xform_point(sc.camera_to_world, V3{0.f, 0.f, 0.f});
    const V3 wo = -d;
    ShadingFrame fr;
    float reps;
    const RenderMaterial *mat = nullptr;
    if (lsurf) {  // Sphere::Intersect: rayEpsilon = 5e-4f * thit (sphere.cpp:155)
        fr = sphere_frame(sc.lights[-1 - tri].s, o, d, ha.x);
        reps = 5e-4f * ha.x;
    } else {
        const RenderMesh &mesh = sc.meshes[sc.tri_mesh[tri]];
        const V3 p = o + d * ha.x;  // Ray::operator()
        reps = 1e-3f * ha.x;
        fr = tri_shading(mesh.view, sc.tri_local[tri], p, 1.f - ha.y - ha.z, ha.y, ha.z);
        mat = &sc.materials[mid];
        if (mat->has_bump) {  // BSDF on the bumped dgs: nn, sn = Normalize(dpdu), tn = Cross(nn, sn)
            const float4 a = rec.hit_frame[2 * (size_t)slot], b = rec.hit_frame[2 * (size_t)slot + 1];
            fr.nn = V3{a.x, a.y, a.z};
            fr.sn = V3{b.x, b.y, b.z};
            fr.tn = cross(fr.nn, fr.sn);
        }
    }
    if (lj == 0) {
        float ct = absdot(wo, fr.nn);
        ct = ct < 1.f ? ct : 1.f;
        rec.hit_q[slot] = make_float4(fr.p.x, fr.p.y, fr.p.z, sss ? ct : -1.f);
        if (j >= ns) return;
    }
    SpecOf<kSpec> bs;
    load_spec(bs, mat, rec, slot);
    const int ncomp = mat ? bs.has_refl() + bs.has_trans() : 1;
    const V3 wo_l = to_local(fr, wo);
    const float ng_wo = dot(wo, fr.ng);
    // LightSample(sample, offsets, j) / BSDFSample(sample, offsets, j) (light.cpp, reflection.cpp)
    float lu0, lu1, ubc, ub0, ub1;
    if (sc.replay) {
        const int px = (int)(pix % (uint32_t)sc.xres), py = (int)(pix / (uint32_t)sc.xres);
        const int k = L.replay_off + j * kReplayPerLightSample;
        lu0 = replay_val(sc, px, py, s, k);
        lu1 = replay_val(sc, px, py, s, k + 1);
        ubc = replay_val(sc, px, py, s, k + 2);
        ub0 = replay_val(sc, px, py, s, k + 3);
        ub1 = replay_val(sc, px, py, s, k + 4);
    } else {
        const uint32_t xr = (spp & (spp - 1)) == 0 ? (hash3(seed, pix, 16u * l + 9u) & (uint32_t)(spp - 1)) : 0u;
        const uint32_t nidx = (uint32_t)(s ^ (int)xr) * (uint32_t)ns + (uint32_t)j;
        lu0 = van_der_corput(nidx, hash3(seed, pix, 16u * l + DIM_LIGHT_POS));
        lu1 = sobol2(nidx, hash3(seed, pix, 16u * l + DIM_LIGHT_POS + 8u));
        ubc = van_der_corput(nidx, hash3(seed, pix, 16u * l + DIM_BSDF_COMP));
        ub0 = van_der_corput(nidx, hash3(seed, pix, 16u * l + DIM_BSDF_DIR));
        ub1 = sobol2(nidx, hash3(seed, pix, 16u * l + DIM_BSDF_DIR + 8u));
    }
    // --- light sampling: ed += f * Li * (|wi.n| * w / lightPdf)
    const LightSampleOut ls = L.kind ? sample_infinite(L, fr.p, reps, lu0, lu1) : sample_light(L, fr.p, reps, lu0, lu1);
    float lightPdf = ls.pdf;
    float4 st = make_float4(ls.ms, ls.mt, 0.f, 0.f);
    if (lightPdf > 0.f && ls.nonblack && ncomp > 0) {
        const V3 wi_l = to_local(fr, ls.wi);
        const Lobe f1 = bsdf_lobe(bs, dot(ls.wi, fr.ng) * ng_wo > 0.f, wo_l, wi_l);
        if (!lobe_black(bs, f1) && !trace_any_wave(sc, ls.so, ls.sd, ls.smint, ls.smaxt, true, false, true)) {
            const float bsdfPdf = bsdf_pdf(bs, wo_l, wi_l);
            const float w = power_heuristic(lightPdf, bsdfPdf);
            out.k1 = absdot(ls.wi, fr.nn) * w / lightPdf;
            out.l1 = f1;
        }
    }
    // --- BSDF sampling (BSDF::Sample_f, reflection.cpp:675-733): ed += f * Li * |wi.n| * w / pdf
    if (ncomp > 0) {
        int which = (int)floorf(ubc * (float)ncomp);
        which = which < ncomp - 1 ? which : ncomp - 1;
        const bool pick_t = mat && (!bs.has_refl() || which == 1);
        V3 wi_l;
        float bsdfPdf;
        if (!mat)
            lambert_sample(wo_l, ub0, ub1, wi_l, bsdfPdf);
        else if (pick_t)
            mt_sample_ool(mat->mf, wo_l, ub0, ub1, wi_l, bsdfPdf);
        else
            beckmann_sample(mat->mf, wo_l, ub0, ub1, wi_l, bsdfPdf);
        if (bsdfPdf != 0.f) {
            const V3 wi = to_world(fr, wi_l);
            if (ncomp > 1) {
                bsdfPdf += pick_t ? microfacet_pdf(mat->mf, wo_l, wi_l) : mt_pdf_ool(mat->mf, wo_l, wi_l);
                bsdfPdf /= (float)ncomp;
            }
            const Lobe f2 = bsdf_lobe(bs, dot(wi, fr.ng) * ng_wo > 0.f, wo_l, wi_l);
            if (!lobe_black(bs, f2) && bsdfPdf > 0.f) {
                lightPdf = L.kind ? infinite_pdf(L, wi) : sphere_pdf(L.s, fr.p, wi);
                if (lightPdf != 0.f) {
                    const float w = power_heuristic(bsdfPdf, lightPdf);
                    // Li = lightIsect.Le(-wi) when Scene::Intersect's closest primitive is this light;
                    // light->Le(ray) when the ray escapes (0 for an area light). Both are answered by
                    // any-hit walks:
                    //  * infinite light: the ray escapes iff it hits no triangle and no light sphere;
                    //  * area light: the ray meets the light only if it meets its sphere at all (the
                    //    sphere test with maxt = inf accepts every hit the closest-hit search would), at
                    //    tl. The closest-hit search from maxt = tl ends on a triangle iff one lies at
                    //    t < tl (at t == tl the spheres, tested last, take over), and otherwise its
                    //    sphere loop alone decides -- so: no triangle before tl (strict any-hit), then
                    //    the sphere loop from tl, exactly as trace_closest runs it.
                    bool lit = false;
                    if (L.kind) {
                        lit = !trace_any_wave(sc, fr.p, wi, reps, INFINITY, true, false, true);
                        if (lit) {
                            inf_coords(L, wi, st.z, st.w);
                            lit = inf_nonblack(L, st.z, st.w);
                        }
                    } else {
                        float tl;
                        if (sphere_hit_ool(L.s, fr.p, wi, reps, INFINITY, tl, nullptr) &&
                            !trace_any_wave(sc, fr.p, wi, reps, tl, true, true, false)) {
                            float ht = tl;
                            int who = INT_MIN;
                            V3 lnn = V3{0.f, 0.f, 0.f};
                            for (int k = 0; k < sc.nlights; ++k) {
                                if (sc.lights[k].kind) continue;
                                float t;
                                V3 nn;
                                if (sphere_hit_ool(sc.lights[k].s, fr.p, wi, reps, ht, t, &nn)) {
                                    ht = t;
                                    who = -1 - k;
                                    lnn = nn;
                                }
                            }
                            lit = who == -1 - l && dot(lnn, -wi) > 0.f;
                        }
                    }
                    if (lit) {
                        out.adn = absdot(wi, fr.nn);
                        out.w2 = w;
                        out.pdf2 = bsdfPdf;
                        out.l2 = f2;
                    }
                }
            }
        }
    }
    terms[gid] = out;
    if (L.kind) inf_st[gid] = st;
}
__global__ __launch_bounds__(256) void shade_direct_kernel(RenderScene sc, SampleRecs rec, int spp, uint32_t seed,
                                                           int max_hits, int ns_max, DirectTerms *terms,
                                                           float4 *__restrict__ inf_st) {
    shade_direct<false>(sc, rec, spp, seed, max_hits, ns_max, terms, inf_st);
}
__global__ __launch_bounds__(256) void shade_direct_spec_kernel(RenderScene sc, SampleRecs rec, int spp, uint32_t seed,
                                                                int max_hits, int ns_max, DirectTerms *terms,
                                                                float4 *__restrict__ inf_st) {
    shade_direct<true>(sc, rec, spp, seed, max_hits, ns_max, terms, inf_st);
}

// ------------------------------------------------------------------ textures
// Li's GetBSDF / GetMultipoleBSSRDF for materials with an albedo texture or a bump map: the
// camera RayDifferential (PerspectiveCamera::GenerateRayDifferential, perspective.cpp:81-113,
// ScaleDifferentials(1 / sqrtf(spp)), samplerrenderer.cpp:90-91), dg.ComputeDifferentials, then
// albedo->Evaluate(dgShading) (layeredskin.cpp:180-185) and Bump (layeredskin.cpp:143-146).
// kSpec (shade_tex_spec_kernel): also Kr->Evaluate(dgs) / Kt->Evaluate(dgs) of GetBSDF (layeredskin.cpp:
// 154-155) for every mesh hit of a material with such a texture. dgs is the bumped geometry, whose u, v and
// differentials are dgShading's (Bump copies them, core/material.cpp:93).
template <bool kSpec>
__device__ __forceinline__ void shade_tex(const RenderScene &sc, const SampleRecs &rec, int spp, uint32_t seed,
                                          int max_hits) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int nhits = *rec.hit_count;
    if (slot >= nhits || slot >= max_hits) return;
    const uint32_t hs = rec.hit_s[slot];
    if (hs & HS_LIGHT) return;
    const RenderMaterial &mat = sc.materials[(hs >> REC_MAT_SHIFT) & 0xffu];
    const bool want_alb = (hs >> 31) && mat.has_alb_tex;
    if (!want_alb && !mat.has_bump && !(kSpec && (mat.has_kr_tex || mat.has_kt_tex))) return;
    const float4 ha = rec.hit_a[slot], hb = rec.hit_b[slot];
    const int s = (int)(hs & 0xffffu), tri = __float_as_int(ha.w);
    const uint32_t pix = __float_as_uint(hb.w);
    const V3 d = V3{hb.x, hb.y, hb.z};
    const V3 o = xform_point(sc.camera_to_world, V3{0.f, 0.f, 0.f});
    const RenderMesh &mesh = sc.meshes[sc.tri_mesh[tri]];
    const V3 p = o + d * ha.x;
    const ShadingFrame fr = tri_shading(mesh.view, sc.tri_local[tri], p, 1.f - ha.y - ha.z, ha.y, ha.z);
    // the sample's image position (as primary_kernel) and its offset rays
    const int px = (int)(pix % (uint32_t)sc.xres), py = (int)(pix / (uint32_t)sc.xres);
    float X, Y;
    image_sample(sc, seed, px, py, s, X, Y);
    const V3 pcam = xform_point(sc.raster_to_camera, V3{X, Y, 0.f});
    const V3 dxc = V3{sc.dx_camera[0], sc.dx_camera[1], sc.dx_camera[2]};
    const V3 dyc = V3{sc.dy_camera[0], sc.dy_camera[1], sc.dy_camera[2]};
    const V3 rxw = xform_vector(sc.camera_to_world, normalize(pcam + dxc));
    const V3 ryw = xform_vector(sc.camera_to_world, normalize(pcam + dyc));
    const float k = 1.f / sqrtf((float)spp);
    const V3 rxd = d + (rxw - d) * k, ryd = d + (ryw - d) * k;
    UVDiff g;
    g.u = fr.u;
    g.v = fr.v;
    compute_differentials(p, fr.ng, fr.dpdu, fr.dpdv, o, rxd, ryd, g);
    if (want_alb) {
        float rgb[3];
        tex_eval(mat.alb_tex, g, rgb);
        rec.hit_alb[slot] = make_float4(rgb[0], rgb[1], rgb[2], 0.f);
    }
    if (mat.has_bump) {
        V3 dpdu_b, nn_b;
        bump_frame(mat.bump_tex, g, fr.ss, fr.ts, fr.dndu, fr.dndv, fr.nn, fr.ng, mesh.view.flip, dpdu_b, nn_b);
        const V3 sn = normalize(dpdu_b);  // BSDF: sn = Normalize(dgs.dpdu)
        rec.hit_frame[2 * (size_t)slot] = make_float4(nn_b.x, nn_b.y, nn_b.z, 0.f);
        rec.hit_frame[2 * (size_t)slot + 1] = make_float4(sn.x, sn.y, sn.z, 0.f);
    }
    if (kSpec) {
        if (mat.has_kr_tex) rec.hit_kr[slot] = spec_lookup(mat.kr_tex, g);
        if (mat.has_kt_tex) rec.hit_kt[slot] = spec_lookup(mat.kt_tex, g);
    }
}
__global__ __launch_bounds__(256) void shade_tex_kernel(RenderScene sc, SampleRecs rec, int spp, uint32_t seed,
                                                        int max_hits) {
    shade_tex<false>(sc, rec, spp, seed, max_hits);
}
__global__ __launch_bounds__(256) void shade_tex_spec_kernel(RenderScene sc, SampleRecs rec, int spp, uint32_t seed,
                                                             int max_hits) {
    shade_tex<true>(sc, rec, spp, seed, max_hits);
}

// A scene without lights: no direct light and (Preprocess returned early) no octree.
__global__ __launch_bounds__(256) void shade_nolight_kernel(RenderScene sc, SampleRecs rec, int max_hits) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int nhits = *rec.hit_count;
    if (slot >= nhits || slot >= max_hits) return;
    rec.hit_q[slot] = make_float4(0.f, 0.f, 0.f, -1.f);
    float4 *row = reinterpret_cast<float4 *>(rec.ld + (size_t)slot * ROW);
    for (int k = 0; k < 8; ++k) row[k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// One test per light sample for the Microfacet half: every band's dividend x = ((R[c] D) G) F and quotient
// x / den lie in div_by's guarded range [2^-100, 2^100] (or x = +0), so the 30 quotients take div_by's fast
// path (RN(x inv) and one Markstein correction) with no per-band range test: the same values. R, D, G, F
// >= 0, so x >= +0. r_lo / r_hi bound R's nonzero values; the factor-2 margins absorb the roundings of
// the bound's own products and of x's (a few ulps).
template <class M>  // M: R's range -- the material's record, or a textured hit's own (HitBands)
__device__ __forceinline__ bool refl_quotients_safe(const M &m, const Lobe &L, const Den &den) {
    if (!den.ok || !m.r_nonneg || !(L.a >= 0.f && L.b >= 0.f && L.c >= 0.f)) return false;
    if (L.a == 0.f || L.b == 0.f || L.c == 0.f || m.r_hi == 0.f) return true;  // every x = +0: q = +-0 exactly
    const float abc = (L.a * L.b) * L.c;
    const float lo = m.r_lo * abc, hi = m.r_hi * abc, ai = fabsf(den.inv);
    return lo >= 0x1p-99f && hi <= 0x1p99f && lo * ai >= 0x1p-99f && hi * ai <= 0x1p99f;
}

// direct_combine's view of a hit's R and T. MatBands: the material's record. HitBands (a scene with Kr / Kt
// textures): R's 30 bands in registers, formed once per hit (every light sample multiplies them), with
// their range for refl_quotients_safe found as upload_materials finds a material's -- a texture with a
// negative shift or a NaN texel is no promise of R >= 0, so r_nonneg is tested band by band; T, read only
// by the rare transmission terms, band by band from the hit's lookup.
struct MatBands {
    const RenderMaterial *mat;
    __device__ __forceinline__ float R(int c) const { return mat->R[c]; }
    __device__ __forceinline__ float T(int c) const { return mat->T[c]; }
    __device__ __forceinline__ const RenderMaterial &range() const { return *mat; }
};
struct HitBands {
    HitSpec h;
    float Rv[NB];
    float r_lo, r_hi;
    int r_nonneg;
    __device__ __forceinline__ float R(int c) const { return Rv[c]; }
    __device__ __forceinline__ float T(int c) const { return h.T(c); }
    __device__ __forceinline__ const HitBands &range() const { return *this; }
};
__device__ __forceinline__ void load_bands(MatBands &b, const RenderMaterial *mat, const SampleRecs &, int) { b.mat = mat; }
__device__ __forceinline__ void load_bands(HitBands &b, const RenderMaterial *mat, const SampleRecs &rec, int slot) {
    load_spec(b.h, mat, rec, slot);
    b.r_lo = INFINITY;
    b.r_hi = 0.f;
    b.r_nonneg = 1;
    bool black = true;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const float r = mat ? b.h.R(c) : 0.f;  // (a light sphere's matte lobe reads no R)
        b.Rv[c] = r;
        if (!(r >= 0.f)) b.r_nonneg = 0;
        if (r > 0.f) b.r_lo = fminf(b.r_lo, r);
        b.r_hi = fmaxf(b.r_hi, r);
        black = black && r == 0.f;
    }
    if (black) b.r_lo = 0.f;
}

// ld[c] = sum over lights of (sum over j of (0 + light term + BSDF term)) / ns, band by band in
// the order UniformSampleAllLights accumulates (Ld += EstimateDirect; L += Ld / nSamples). Each
// light sample's record is read once and added to all 30 per-band accumulators (registers);
// every band sees exactly the reference's sequence of float operations. kInf: the scene has
// infinite lights, whose radiance depends on each term's direction (map coordinates in inf_st).
// kSpec: R and T are the hit's own (HitBands) -- direct_combine_spec_kernel.
template <bool kInf, bool kSpec>
__device__ __forceinline__ void direct_combine(const RenderScene &sc, const SampleRecs &rec, int max_hits, int ns_max,
                                               const DirectTerms *__restrict__ terms,
                                               const float4 *__restrict__ inf_st) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int nhits = *rec.hit_count;
    if (slot >= nhits || slot >= max_hits) return;
    const uint32_t hs = rec.hit_s[slot];
    if ((hs & HS_LIGHT) && !(hs & HS_LSURF)) return;
    // a light sphere's surface: the matte lobe (kind 3) needs no material
    const RenderMaterial *mat = (hs & HS_LIGHT) ? nullptr : &sc.materials[(hs >> REC_MAT_SHIFT) & 0xffu];
    std::conditional_t<kSpec, HitBands, MatBands> bd;
    load_bands(bd, mat, rec, slot);
    const size_t base = (size_t)slot * sc.nlights * ns_max;
    float ld[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) ld[c] = 0.f;
    for (int l = 0; l < sc.nlights; ++l) {
        const RenderLight &L = sc.lights[l];
        const int ns = L.nsamples_round;
        float Ld[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) Ld[c] = 0.f;
        for (int j = 0; j < ns; ++j) {
            const DirectTerms e = terms[base + l * ns_max + j];
            if (!e.l1.kind && !e.l2.kind) continue;  // ed = 0 and Ld += 0 changes nothing (Ld is never -0)
            float rgb1[3], rgb2[3];
            const bool inf = kInf && L.kind;
            if (inf) {  // Spectrum(map lookup, SPECTRUM_ILLUMINANT) at each term's direction
                const float4 st = inf_st[base + l * ns_max + j];
                inf_lookup(L, st.x, st.y, rgb1);
                inf_lookup(L, st.z, st.w, rgb2);
            }
            const Den d1 = make_den(e.l1.d), d2 = make_den(e.l2.d), dp = make_den(e.pdf2);
            if (!e.l2.kind && e.l1.kind == 1u && refl_quotients_safe(bd.range(), e.l1, d1)) {
                // the common term: a Microfacet light-sample half alone, its quotients on the fast path
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const float Li1 = inf ? illum_band(rgb1, c) : L.Lemit[c];
                    const float x = bd.R(c) * e.l1.a * e.l1.b * e.l1.c;
                    const float q = x * d1.inv;
                    const float f1 = __builtin_fmaf(__builtin_fmaf(-d1.d, q, x), d1.inv, q);
                    Ld[c] += 0.f + f1 * Li1 * e.k1;
                }
                continue;
            }
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const float Li1 = inf ? illum_band(rgb1, c) : L.Lemit[c];
                const float Li2 = inf ? illum_band(rgb2, c) : L.Lemit[c];
                float ed = 0.f;
                if (e.l1.kind) ed += lobe_value_den(bd, e.l1, c, d1) * Li1 * e.k1;
                if (e.l2.kind) ed += div_by(lobe_value_den(bd, e.l2, c, d2) * Li2 * e.adn * e.w2, dp.d, dp.inv, dp.ok);
                Ld[c] += ed;
            }
        }
        // L += Ld / nSamples. nsamples_round is a power of two (LDSampler::RoundSize), and x / 2^k and
        // x * 2^-k are the same exact real rounded once, for every x (subnormal results included)
        if ((ns & (ns - 1)) == 0) {
            const float inv_ns = 1.f / (float)ns;
#pragma unroll
            for (int c = 0; c < NB; ++c) ld[c] += Ld[c] * inv_ns;
        } else {
            const Den dn = make_den((float)ns);
#pragma unroll
            for (int c = 0; c < NB; ++c) ld[c] += div_by(Ld[c], dn.d, dn.inv, dn.ok);
        }
    }
    float4 *row = reinterpret_cast<float4 *>(rec.ld + (size_t)slot * ROW);
#pragma unroll
    for (int k = 0; k < 7; ++k) row[k] = make_float4(ld[4 * k], ld[4 * k + 1], ld[4 * k + 2], ld[4 * k + 3]);
    row[7] = make_float4(ld[28], ld[29], 0.f, 0.f);
}
template <bool kInf>
__global__ __launch_bounds__(256) void direct_combine_kernel(RenderScene sc, SampleRecs rec, int max_hits, int ns_max,
                                                             const DirectTerms *__restrict__ terms,
                                                             const float4 *__restrict__ inf_st) {
    direct_combine<kInf, false>(sc, rec, max_hits, ns_max, terms, inf_st);
}
template <bool kInf>
__global__ __launch_bounds__(256) void direct_combine_spec_kernel(RenderScene sc, SampleRecs rec, int max_hits,
                                                                  int ns_max, const DirectTerms *__restrict__ terms,
                                                                  const float4 *__restrict__ inf_st) {
    direct_combine<kInf, true>(sc, rec, max_hits, ns_max, terms, inf_st);
}
template __global__ void direct_combine_kernel<false>(RenderScene, SampleRecs, int, int, const DirectTerms *,
                                                      const float4 *);
template __global__ void direct_combine_kernel<true>(RenderScene, SampleRecs, int, int, const DirectTerms *,
                                                     const float4 *);
template __global__ void direct_combine_spec_kernel<false>(RenderScene, SampleRecs, int, int, const DirectTerms *,
                                                           const float4 *);
template __global__ void direct_combine_spec_kernel<true>(RenderScene, SampleRecs, int, int, const DirectTerms *,
                                                          const float4 *);

}  // namespace mpss
