// preprocess_kernels.hip -- MultipoleSubsurfaceIntegrator::Preprocess on the GPU, once per scene and
// before any render batch (DESIGN.md "A render batch" starts after it; the tessellation kernel is in
// tess_kernel.h):
//   irradiance_kernel         IrradianceTask::Run (integrators/multipolesubsurface.cpp:156-236 [file])
//   poisson_walk_kernel       SurfacePointTask::Run's paths (renderers/surfacepoints.cpp:181-215)
//   replay_irradiance_kernel  IrradianceTask's RNG(47 k) scrambles in reference-sampler mode
// Sample values come from counter-based scrambled (0,2)-sequences (pbrt_math.h), identical in the
// CPU oracle ("replay mode").
#include "render.h"

#include <climits>

#include "bvh_trace.h"
#include "geom.h"
#include "light_sample.h"
#include "spectrum_tables.h"

namespace mpss {

// ------------------------------------------------------------------ irradiance (Preprocess)
__global__ __launch_bounds__(256) void irradiance_kernel(RenderScene sc, const float *__restrict__ sp_p,
                                                         const float *__restrict__ sp_n,
                                                         const float *__restrict__ sp_eps,
                                                         const uint32_t *__restrict__ sp_mat,
                                                         const float *__restrict__ sp_uv, int n, uint32_t seed,
                                                         float *__restrict__ E_out) {
    __shared__ int stk_all[kTraceStack * 256];
    int *stk = stk_all + threadIdx.x;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 p = V3{sp_p[3 * i], sp_p[3 * i + 1], sp_p[3 * i + 2]};
    const V3 nrm = V3{sp_n[3 * i], sp_n[3 * i + 1], sp_n[3 * i + 2]};
    const float eps = sp_eps[i];
    const uint32_t mid = sp_mat[i];
    const bool has_mat = mid < (uint32_t)sc.nmaterials;
    const RenderMaterial *mat = has_mat ? &sc.materials[mid] : nullptr;
    const bool bss = has_mat && mat->has_bssrdf;
    float E[NB];
    for (int c = 0; c < NB; ++c) E[c] = 0.f;
    for (int l = 0; l < sc.nlights; ++l) {
        const RenderLight &L = sc.lights[l];
        float El[NB];
        for (int c = 0; c < NB; ++c) El[c] = 0.f;
        const int ns = L.nsamples_pow2;
        uint32_t scr0, scr1;
        if (sc.irr_scr) {  // the reference's RNG(47 k) stream (replay_irradiance_kernel)
            scr0 = sc.irr_scr[((size_t)i * sc.nlights + l) * 2];
            scr1 = sc.irr_scr[((size_t)i * sc.nlights + l) * 2 + 1];
        } else {
            scr0 = hash3(seed, (uint32_t)i, 16u * l + DIM_IRR_POS);
            scr1 = hash3(seed, (uint32_t)i, 16u * l + DIM_IRR_POS + 8u);
        }
        for (int s = 0; s < ns; ++s) {
            const float u0 = van_der_corput((uint32_t)s, scr0), u1 = sobol2((uint32_t)s, scr1);  // Sample02
            const LightSampleOut ls = L.kind ? sample_infinite(L, p, eps, u0, u1) : sample_light(L, p, eps, u0, u1);
            if (dot(ls.wi, nrm) <= 0.f) continue;
            if (!ls.nonblack || ls.pdf == 0.f) continue;
            if (!trace_any(sc, ls.so, ls.sd, ls.smint, ls.smaxt, stk, 256)) {
                float ct = absdot(ls.wi, nrm);
                ct = ct < 1.f ? ct : 1.f;
                const float Ft = bss ? 1.f - rho_lookup(mat->rho, mat->n_rho, ct) : 1.f;
                if (L.kind) {  // Li = Spectrum(map lookup at the sampled uv, SPECTRUM_ILLUMINANT)
                    float rgb[3];
                    inf_lookup(L, ls.ms, ls.mt, rgb);
                    for (int c = 0; c < NB; ++c) El[c] += Ft * illum_band(rgb, c) * ct / ls.pdf;
                } else {
                    for (int c = 0; c < NB; ++c) El[c] += Ft * L.Lemit[c] * ct / ls.pdf;
                }
            }
        }
        for (int c = 0; c < NB; ++c) E[c] += El[c] / (float)ns;
    }
    if (bss && mat->has_alb_tex) {  // albedo->Evaluate(dgs): dgs has no differentials -> triangle(0, s, t)
        const UVDiff g{sp_uv[2 * i], sp_uv[2 * i + 1], 0.f, 0.f, 0.f, 0.f};
        float rgb[3];
        tex_eval(mat->alb_tex, g, rgb);
        for (int c = 0; c < NB; ++c) E[c] *= tex_albedo_pow(rgb, c, mat->mix);
    } else if (bss) {
        for (int c = 0; c < NB; ++c) E[c] *= mat->alb_mix[c];
    }
    for (int c = 0; c < NB; ++c) E_out[(size_t)i * NB + c] = E[c];
}

// ------------------------------------------------------------------ Poisson point finder
// SurfacePointTask::Run's paths (renderers/surfacepoints.cpp:181-215): from pCamera in a
// uniformly random direction, up to 30 rays; a ray that leaves the scene bounces off the inside
// of the bounding sphere; hits of rays of depth >= 3 on a surface whose material has a BSSRDF
// become candidate SurfacePoints (p, shading normal, u, v, material, area, rayEpsilon); each
// next direction is a uniform sphere sample turned to the faceforwarded normal. Random numbers
// are counter-based per (seed, path, draw) -- replay mode, like the render sampler.
__device__ __forceinline__ float poisson_u01(uint32_t seed, uint32_t path, uint32_t k) {
    return (float)(hash3(seed, path, k) >> 8) * 0x1p-24f;
}
__device__ __forceinline__ V3 sphere_hit_point(const SphereView &s, V3 o, V3 d, float t) {
    V3 ph = (o - s.c) + d * t;  // object-space Ray::operator() of the translated sphere
    if (ph.x == 0.f && ph.y == 0.f) ph.x = 1e-5f * s.r;
    return ph + s.c;
}
__device__ __forceinline__ V3 faceforward(V3 n, V3 v) { return dot(n, v) < 0.f ? -n : n; }

__global__ __launch_bounds__(256) void poisson_walk_kernel(RenderScene sc, PoissonWalk w, SurfacePoint *out,
                                                           int *count) {
    __shared__ int stk_all[kTraceStack * 256];
    int *stk = stk_all + threadIdx.x;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.npaths) return;
    const uint32_t path = w.path0 + (uint32_t)i;
    uint32_t k = 0;
    float u1 = poisson_u01(w.seed, path, k++), u2 = poisson_u01(w.seed, path, k++);
    V3 o = w.origin, d = uniform_sample_sphere(u1, u2);
    float mint = 0.f;
    int n = 0;
    SurfacePoint *mine = out + (size_t)i * kPoissonCand;
    for (int depth = 0; depth < kPoissonDepth; ++depth) {
        const Hit h = trace_closest(sc, o, d, mint, INFINITY, stk, 256);
        V3 p, nn;
        float eps;
        if (h.tri == INT_MIN) {  // sphere.Intersect(ray, &isect): the bounding sphere
            float t;
            V3 snn;
            if (!sphere_intersect(w.bound, o, d, mint, INFINITY, t, &snn)) break;
            p = sphere_hit_point(w.bound, o, d, t);
            nn = snn;
            eps = 5e-4f * t;
            nn = faceforward(nn, -d);
        } else if (h.tri < 0) {  // an area light's sphere (its material has no BSSRDF)
            p = sphere_hit_point(sc.lights[-1 - h.tri].s, o, d, h.t);
            nn = faceforward(h.lnn, -d);
            eps = 5e-4f * h.t;
        } else {
            const int mi = sc.tri_mesh[h.tri], lt = sc.tri_local[h.tri];
            const RenderMesh &mesh = sc.meshes[mi];
            p = o + d * h.t;
            const ShadingFrame fr = tri_shading(mesh.view, lt, p, 1.f - h.b1 - h.b2, h.b1, h.b2);
            nn = faceforward(fr.ng, -d);
            eps = 1e-3f * h.t;
            // every mesh material is a LayeredSkin, whose GetBSSRDF is never NULL (layeredskin.cpp:170-177;
            // surfacepoints.cpp:202) -- genprofile false included: its points are candidates too
            if (depth >= 3 && mesh.material < (uint32_t)sc.nmaterials) {
                // dgs = Bump(hitGeometry, dgShading); without N and S the shading geometry is dg itself
                // (its nn already faceforwarded); no ray differentials (GetBSSRDF(RayDifferential(ray)))
                V3 sn = (!mesh.view.N && !mesh.view.S) ? nn : fr.nn;
                const RenderMaterial &mt = sc.materials[mesh.material];
                if (mt.has_bump) {
                    const UVDiff g{fr.u, fr.v, 0.f, 0.f, 0.f, 0.f};
                    V3 dpdu_b;
                    bump_frame(mt.bump_tex, g, fr.ss, fr.ts, fr.dndu, fr.dndv, sn, nn, mesh.view.flip, dpdu_b, sn);
                }
                SurfacePoint sp;
                sp.p[0] = p.x;
                sp.p[1] = p.y;
                sp.p[2] = p.z;
                sp.n[0] = sn.x;
                sp.n[1] = sn.y;
                sp.n[2] = sn.z;
                sp.u = fr.u;
                sp.v = fr.v;
                sp.material = mesh.material;
                sp.area = 0.f;  // pi (minDist / 2)^2, set by the host
                sp.ray_eps = eps;
                mine[n++] = sp;
            }
        }
        u1 = poisson_u01(w.seed, path, k++);
        u2 = poisson_u01(w.seed, path, k++);
        d = faceforward(uniform_sample_sphere(u1, u2), nn);
        o = p;
        mint = eps;
    }
    count[i] = n;
}

// ------------------------------------------------------------------ reference-sampler replay
// (the render tasks' streams: replay_gen.hip)

// IrradianceTask::Run's RNG(47 k) (multipolesubsurface.cpp:81, 110-112): per point of the task's
// slice and per light, scramble[0], scramble[1], compScramble
__global__ __launch_bounds__(64) void replay_irradiance_kernel(int n, int nlights, int ntasks, uint32_t *mt,
                                                               uint32_t *scr) {
    const int task = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (task >= ntasks) return;
    const int i0 = (int)((uint64_t)task * (uint64_t)n / (uint64_t)ntasks);
    const int i1 = (int)((uint64_t)(task + 1) * (uint64_t)n / (uint64_t)ntasks);
    if (i0 == i1) return;
    Mt19937 rng{mt + task, ntasks, 624};
    rng.seed((uint32_t)task * 47u);
    for (int i = i0; i < i1; ++i)
        for (int l = 0; l < nlights; ++l) {
            uint32_t *o = scr + ((size_t)i * nlights + l) * 2;
            o[0] = rng.next();
            o[1] = rng.next();
            rng.skip(1);  // compScramble (a LightSample's component: one shape per light here)
        }
}

}  // namespace mpss
