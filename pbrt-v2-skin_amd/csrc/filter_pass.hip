// filter_pass.hip -- the camera pass and the texture lookups of a render batch under a non-default pixel
// filter (pixel_filter.h, DESIGN.md "Pixel filters"):
//   primary_filter_kernel    primary_kernel (primary.hip) over pieces of the film's sample extent
//   shade_tex_filter_kernel  shade_tex_kernel (shade.hip) for hits of such pieces, and its instance
//                            shade_tex_filter_spec_kernel (shade_tex_spec_kernel) for Kr / Kt textures
// Each follows its model line for line except where the filter shows, marked "filter:" below. They are
// kernels of their own, in a unit of their own, so that the default filter's kernels keep their code
// objects to the instruction (as instances of one template the default kernels came out reordered).
#include <climits>

#include "bvh_trace.h"
#include "film_filter.h"
#include "geom.h"
#include "spectrum_tables.h"
#include "texture.h"

namespace mpss {

__global__ __launch_bounds__(256) void primary_filter_kernel(RenderScene sc, PieceList pl, SampleRecs rec,
                                                             FilterGeom fg) {
    __shared__ int snode_all[kTraceStack * 4];  // one traversal stack per wave (trace_closest_wave)
    __shared__ uint64_t smask_all[kTraceStack * 4];
    const int wv = (int)(threadIdx.x >> 6);
    const int k = piece_of(pl, (int)blockIdx.x);
    const TileBatch &tb = pl.tb[k];
    rec.flags += pl.off[k];
    rec.slot += pl.off[k];
    const int64_t sid0 = (int64_t)((int)blockIdx.x - pl.block0[k]) * blockDim.x + threadIdx.x;
    const bool in_range = sid0 < tb.nsamples;
    const int64_t sid = in_range ? sid0 : tb.nsamples - 1;
    const int s = (int)(sid % tb.spp);
    const int li = (int)(sid / tb.spp);
    // filter: a pixel of the sample extent, maybe outside the frame; its sampler key (hit_b.w below)
    const int px = tb.ex0 + li % tb.ew, py = tb.ey0 + li / tb.ew;
    const uint32_t pix = filter_pixel_key(fg, sc.xres, sc.yres, px, py);
    float X, Y;
    image_sample_keyed(tb.seed, pix, px, py, s, X, Y);
    // filter: a sample is live when its range meets the tile; no edge bits (film_filter_kernel tests
    // every sample's range itself)
    int lx, hx, ly, hy;
    filter_range(X, fg.wx, sc.xres, lx, hx);
    filter_range(Y, fg.wy, sc.yres, ly, hy);
    const bool live = in_range && lx < tb.x1 && hx >= tb.x0 && ly < tb.y1 && hy >= tb.y0;
    uint32_t flags = 0;
    V3 d = V3{1.f, 1.f, 1.f};
    const V3 o = xform_point(sc.camera_to_world, V3{0.f, 0.f, 0.f});
    if (live) {
        flags |= REC_LIVE;
        // PerspectiveCamera::GenerateRay (cameras/perspective.cpp)
        const V3 pcam = xform_point(sc.raster_to_camera, V3{X, Y, 0.f});
        d = xform_vector(sc.camera_to_world, normalize(pcam));
    }
    // Scene::Intersect, the wave's rays as sign packets (one pixel's samples share one packet)
    const Hit h = trace_closest_wave(sc, o, d, 0.f, INFINITY, live, snode_all + kTraceStack * wv,
                                     smask_all + kTraceStack * wv);
    if (live) {
        if (h.tri == INT_MIN) {  // SamplerRenderer::Li: Li += lights[i]->Le(ray) for every light
            if (sc.n_infinite > 0) flags |= REC_LE | (0xffu << REC_LIGHT_SHIFT);
        } else if (h.tri < 0) {  // an area light's own sphere: Le(wo) if it faces wo, then matte shading
            const int l = -1 - h.tri;
            flags |= REC_LSURF | ((uint32_t)l << REC_LIGHT_SHIFT);
            if (dot(h.lnn, -d) > 0.f) flags |= REC_LE;
        } else {
            const uint32_t mid = sc.meshes[sc.tri_mesh[h.tri]].material;
            flags |= REC_SURF | (mid << REC_MAT_SHIFT);
            if (sc.materials[mid].has_bssrdf && sc.have_octree) flags |= REC_SSS;
        }
    }
    // every sample with radiance (a surface hit, or an area light seen directly) gets a slot
    const bool surf = (flags & REC_SURF) != 0, has_l = surf || (flags & (REC_LE | REC_LSURF));
    const uint64_t m = __builtin_amdgcn_ballot_w64(has_l);
    const int lane = (int)(threadIdx.x & 63);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(rec.hit_count, (int)__builtin_popcountll(m));
    base = __shfl(base, 0);
    const int slot = base + (int)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (!in_range) return;
    rec.flags[sid] = flags;
    rec.slot[sid] = has_l ? slot : -1;
    if (surf) {
        rec.hit_a[slot] = make_float4(h.t, h.b1, h.b2, __int_as_float(h.tri));
        rec.hit_b[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(pix));
        rec.hit_s[slot] = (uint32_t)s | (flags & (0xffu << REC_MAT_SHIFT)) | ((flags & REC_SSS) ? HS_SSS : 0u);
    } else if (has_l) {
        rec.hit_s[slot] = (uint32_t)s | (((flags >> REC_LIGHT_SHIFT) & 0xffu) << REC_MAT_SHIFT) | HS_LIGHT |
                          ((flags & REC_LSURF) ? HS_LSURF : 0u) | ((flags & REC_LE) ? HS_LE : 0u);
        rec.hit_b[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(pix));
        if (flags & REC_LSURF) rec.hit_a[slot] = make_float4(h.t, 0.f, 0.f, __int_as_float(h.tri));
    }
}

template <bool kSpec>
__device__ __forceinline__ void shade_tex_filter(const RenderScene &sc, const SampleRecs &rec, int spp, uint32_t seed,
                                                 int max_hits, const FilterGeom &fg) {
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
    // filter: the pixel of the sampler key, then the sample's image position and its offset rays
    int px, py;
    filter_key_pixel(fg, sc.xres, sc.yres, pix, px, py);
    float X, Y;
    image_sample_keyed(seed, pix, px, py, s, X, Y);
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
__global__ __launch_bounds__(256) void shade_tex_filter_kernel(RenderScene sc, SampleRecs rec, int spp, uint32_t seed,
                                                               int max_hits, FilterGeom fg) {
    shade_tex_filter<false>(sc, rec, spp, seed, max_hits, fg);
}
__global__ __launch_bounds__(256) void shade_tex_filter_spec_kernel(RenderScene sc, SampleRecs rec, int spp,
                                                                    uint32_t seed, int max_hits, FilterGeom fg) {
    shade_tex_filter<true>(sc, rec, spp, seed, max_hits, fg);
}

}  // namespace mpss
