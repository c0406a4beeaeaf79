// primary.hip -- the camera pass, step 1 of a render batch (DESIGN.md "A render batch"), and the
// tile-cost probe the tile planner runs before the first batch:
//   primary_kernel  SamplerRendererTask::Run's head: Camera::GenerateRay -> Scene::Intersect
//                   (renderers/samplerrenderer.cpp:60-167, cameras/perspective.cpp,
//                    accelerators/bvh.cpp:388-488), and compacts the samples with radiance into hit slots
//   probe_kernel    the same ray through each pixel's centre, classified for the tile costs
#include "render.h"

#include <climits>

#include "bvh_trace.h"
#include "geom.h"
#include "pixel_sample.h"

namespace mpss {

// ------------------------------------------------------------------ camera rays (primary)
// SamplerRendererTask::Run's per-sample head: image sample -> PerspectiveCamera::GenerateRay ->
// Scene::Intersect. Surface hits are compacted (one atomic per wave, sample order kept inside
// the wave) so the shading kernel runs on full waves; a miss or an area-light hit ends here.
__global__ __launch_bounds__(256) void primary_kernel(RenderScene sc, PieceList pl, SampleRecs rec) {
    __shared__ int snode_all[kTraceStack * 4];  // one traversal stack per wave (trace_closest_wave)
    __shared__ uint64_t smask_all[kTraceStack * 4];
    const int wv = (int)(threadIdx.x >> 6);
    const int k = piece_of(pl, (int)blockIdx.x);
    const TileBatch &tb = pl.tb[k];
    rec.flags += pl.off[k];
    rec.slot += pl.off[k];
    rec.spill += pl.off[k] / tb.spp;
    const int64_t sid0 = (int64_t)((int)blockIdx.x - pl.block0[k]) * blockDim.x + threadIdx.x;
    const bool in_range = sid0 < tb.nsamples;
    const int64_t sid = in_range ? sid0 : tb.nsamples - 1;
    const int s = (int)(sid % tb.spp);
    const int li = (int)(sid / tb.spp);
    const int px = tb.ex0 + li % tb.ew, py = tb.ey0 + li / tb.ew;
    const uint32_t pix = (uint32_t)py * (uint32_t)sc.xres + (uint32_t)px;
    // image sample (LDPixelSample's imageSamples, montecarlo.cpp:200-250): imageX = x + u in float
    float X, Y;
    image_sample(sc, tb.seed, px, py, s, X, Y);
    // border samples matter only when the box filter carries them into the tile (film_kernel)
    int lx, hx, ly, hy;
    film_extent(X, sc.xres, lx, hx);
    film_extent(Y, sc.yres, ly, hy);
    const bool live = in_range && lx < tb.x1 && hx >= tb.x0 && ly < tb.y1 && hy >= tb.y0;
    uint32_t flags = 0;
    V3 d = V3{1.f, 1.f, 1.f};
    const V3 o = xform_point(sc.camera_to_world, V3{0.f, 0.f, 0.f});
    if (live) {
        flags |= REC_LIVE;
        const uint32_t edge = (lx < px ? REC_XLO : 0u) | (hx > px ? REC_XHI : 0u) | (ly < py ? REC_YLO : 0u) |
                              (hy > py ? REC_YHI : 0u);
        if (edge) {
            flags |= edge;
            atomicOr(&rec.spill[li], edge);
        }
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
        } else if (h.tri != INT_MIN) {
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
        // sample index (16 bits) | material (8 bits) | SSS bit 31
        rec.hit_s[slot] = (uint32_t)s | (flags & (0xffu << REC_MAT_SHIFT)) | ((flags & REC_SSS) ? HS_SSS : 0u);
    } else if (has_l) {
        // a light seen directly: light index (0xff = the infinite lights of a miss); a light sphere's
        // surface is also shaded (HS_LSURF), its Le counted when it faces the ray (HS_LE)
        rec.hit_s[slot] = (uint32_t)s | (((flags >> REC_LIGHT_SHIFT) & 0xffu) << REC_MAT_SHIFT) | HS_LIGHT |
                          ((flags & REC_LSURF) ? HS_LSURF : 0u) | ((flags & REC_LE) ? HS_LE : 0u);
        rec.hit_b[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(pix));
        if (flags & REC_LSURF) rec.hit_a[slot] = make_float4(h.t, 0.f, 0.f, __int_as_float(h.tri));
    }
}

// ------------------------------------------------------------------ tile-cost probe
// PerspectiveCamera::GenerateRay through the pixel centre and Scene::Intersect, as primary_kernel.
__global__ __launch_bounds__(256) void probe_kernel(RenderScene sc, int x0, int x1, int y0, int y1, uint8_t *cls) {
    __shared__ int stk_all[kTraceStack * 256];
    int *stk = stk_all + threadIdx.x;
    const int w = x1 - x0;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= w * (y1 - y0)) return;
    const int px = x0 + i % w, py = y0 + i / w;
    const V3 pcam = xform_point(sc.raster_to_camera, V3{(float)px + 0.5f, (float)py + 0.5f, 0.f});
    const V3 o = xform_point(sc.camera_to_world, V3{0.f, 0.f, 0.f});
    const V3 d = xform_vector(sc.camera_to_world, normalize(pcam));
    const Hit h = trace_closest(sc, o, d, 0.f, INFINITY, stk, 256);
    uint8_t c = 0;
    if (h.tri >= 0) {
        const uint32_t mid = sc.meshes[sc.tri_mesh[h.tri]].material;
        c = (sc.materials[mid].has_bssrdf && sc.have_octree) ? 2 : 1;
    }
    cls[i] = c;
}

}  // namespace mpss
