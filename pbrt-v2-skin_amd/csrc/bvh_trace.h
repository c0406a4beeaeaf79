// bvh_trace.h -- the BVH tracers of the render kernels (preprocess_kernels.hip, primary.hip,
// shade.hip) and the reference-sampler replay generator (replay_gen.hip): the node-bounds test,
// Scene::Intersect and Scene::IntersectP, each per lane and per wave.
#pragma once
#include "geom.h"
#include "mo_band.h"
#include "render.h"

#include <climits>

namespace mpss {

constexpr int kTraceStack = 48;  // BVH traversal stack depth (host checks the tree depth)

// ------------------------------------------------------------------ BVH traversal (per lane)
__device__ __forceinline__ bool bbox_hit(const BvhNode &n, V3 o, V3 inv, const int neg[3], float mint, float maxt) {
    // bvh.cpp:126-148 (IntersectP of a node's bounds)
    const float *lo = n.bmin, *hi = n.bmax;
    float tmin = ((neg[0] ? hi[0] : lo[0]) - o.x) * inv.x;
    float tmax = ((neg[0] ? lo[0] : hi[0]) - o.x) * inv.x;
    const float tymin = ((neg[1] ? hi[1] : lo[1]) - o.y) * inv.y;
    const float tymax = ((neg[1] ? lo[1] : hi[1]) - o.y) * inv.y;
    if ((tmin > tymax) || (tymin > tmax)) return false;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    const float tzmin = ((neg[2] ? hi[2] : lo[2]) - o.z) * inv.z;
    const float tzmax = ((neg[2] ? lo[2] : hi[2]) - o.z) * inv.z;
    if ((tmin > tzmax) || (tzmin > tmax)) return false;
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmax) tmax = tzmax;
    return (tmin < maxt) && (tmax > mint);
}

namespace {
struct Hit {
    float t, b1, b2;
    int tri;    // global triangle id (>= 0) or -1 - light index, or INT_MIN for a miss
    V3 lnn;     // light-sphere dg.nn when a light is hit
};

// Scene::Intersect: BVH triangles + every sphere light (closest hit, bvh.cpp:388-439).
__device__ Hit trace_closest(const RenderScene &sc, V3 o, V3 d, float mint, float maxt, int *stk, int sstride) {
    Hit h;
    h.tri = INT_MIN;
    h.t = maxt;
    const V3 inv = V3{1.f / d.x, 1.f / d.y, 1.f / d.z};
    const int neg[3] = {inv.x < 0.f, inv.y < 0.f, inv.z < 0.f};
    int todo = 0, node = 0;
    for (;;) {
        const BvhNode n = sc.bvh[node];
        if (bbox_hit(n, o, inv, neg, mint, h.t)) {
            if (n.nprims > 0) {
                for (int i = 0; i < n.nprims; ++i) {
                    const TriRec tr = sc.tris[n.offset + i];
                    float t, b1, b2;
                    if (tri_intersect(o, d, mint, h.t, V3{tr.p1[0], tr.p1[1], tr.p1[2]},
                                      V3{tr.e1[0], tr.e1[1], tr.e1[2]}, V3{tr.e2[0], tr.e2[1], tr.e2[2]}, t, b1, b2)) {
                        h.t = t;
                        h.b1 = b1;
                        h.b2 = b2;
                        h.tri = tr.tri;
                    }
                }
                if (todo == 0) break;
                node = stk[--todo * sstride];
            } else if (neg[n.axis]) {
                stk[todo++ * sstride] = node + 1;
                node = n.offset;
            } else {
                stk[todo++ * sstride] = n.offset;
                node = node + 1;
            }
        } else {
            if (todo == 0) break;
            node = stk[--todo * sstride];
        }
    }
    for (int l = 0; l < sc.nlights; ++l) {
        if (sc.lights[l].kind) continue;  // an infinite light has no shape
        float t;
        V3 nn;
        if (sphere_intersect(sc.lights[l].s, o, d, mint, h.t, t, &nn)) {
            h.t = t;
            h.tri = -1 - l;
            h.lnn = nn;
        }
    }
    return h;
}
}  // namespace

// Scene::IntersectP (bvh.cpp:442-488 + Sphere::IntersectP)
__device__ inline bool trace_any(const RenderScene &sc, V3 o, V3 d, float mint, float maxt, int *stk, int sstride) {
    for (int l = 0; l < sc.nlights; ++l) {
        float t;
        if (!sc.lights[l].kind && sphere_intersect(sc.lights[l].s, o, d, mint, maxt, t, nullptr)) return true;
    }
    const V3 inv = V3{1.f / d.x, 1.f / d.y, 1.f / d.z};
    const int neg[3] = {inv.x < 0.f, inv.y < 0.f, inv.z < 0.f};
    int todo = 0, node = 0;
    for (;;) {
        const BvhNode n = sc.bvh[node];
        if (bbox_hit(n, o, inv, neg, mint, maxt)) {
            if (n.nprims > 0) {
                for (int i = 0; i < n.nprims; ++i) {
                    const TriRec tr = sc.tris[n.offset + i];
                    float t, b1, b2;
                    if (tri_intersect(o, d, mint, maxt, V3{tr.p1[0], tr.p1[1], tr.p1[2]},
                                      V3{tr.e1[0], tr.e1[1], tr.e1[2]}, V3{tr.e2[0], tr.e2[1], tr.e2[2]}, t, b1, b2))
                        return true;
                }
                if (todo == 0) break;
                node = stk[--todo * sstride];
            } else if (neg[n.axis]) {
                stk[todo++ * sstride] = node + 1;
                node = n.offset;
            } else {
                stk[todo++ * sstride] = n.offset;
                node = node + 1;
            }
        } else {
            if (todo == 0) break;
            node = stk[--todo * sstride];
        }
    }
    return false;
}

namespace {
// Sphere::Intersect out of line: its double-precision atan2 (the phi test) would otherwise set the
// register budget of every kernel that inlines a light loop.
__device__ __noinline__ bool sphere_hit_ool(const SphereView &s, V3 o, V3 d, float mint, float maxt, float &thit,
                                            V3 *nn) {
    return sphere_intersect(s, o, d, mint, maxt, thit, nn);
}

// ------------------------------------------------------------------ BVH traversal (per wave)
// The hot kernels trace with the whole wave walking one node sequence: the node index is
// wave-uniform, so node and triangle records are scalar loads, and no lane carries a stack.

// Scene::Intersect's BVH part (bvh.cpp:388-439) for the active lanes whose rays share the direction
// signs (dirIsNeg) of `pat`: with the signs shared, every lane's ordered traversal (near child first)
// visits its nodes in one common order, so the wave walks the union with one stack of (node, lane
// mask) entries in LDS; a lane enters a node only if it is in the entry's mask and hits the box with
// its own current t. Each lane therefore tests exactly the nodes and triangles, in exactly the
// order, of its own traversal, and ends with the same hit.
__device__ void trace_closest_packet(const RenderScene &sc, V3 o, V3 inv, const int neg[3], V3 d, float mint, Hit &h,
                                     uint64_t grp, int pat, int *snode, uint64_t *smask) {
    const int lane = (int)(threadIdx.x & 63);
    const bool mine = (grp >> lane) & 1ull;
    const cptr<BvhNode> nodes = as_const(sc.bvh);
    const cptr<TriRec> tris = as_const(sc.tris);
    int node = 0, sp = 0;
    uint64_t mask = grp;
    for (;;) {
        node = __builtin_amdgcn_readfirstlane(node);
        const BvhNode n = nodes[node];
        const bool in = mine && ((mask >> lane) & 1ull) && bbox_hit(n, o, inv, neg, mint, h.t);
        const uint64_t m = __builtin_amdgcn_ballot_w64(in);
        if (m != 0 && n.nprims == 0) {  // interior: near child now, far child on the stack
            const int a = (int)n.axis;
            const bool far_first = ((pat >> a) & 1) != 0;  // dirIsNeg[axis]: the second child is near
            snode[sp] = far_first ? node + 1 : n.offset;
            smask[sp] = m;
            ++sp;
            node = far_first ? n.offset : node + 1;
            mask = m;
            continue;
        }
        if (m != 0) {  // leaf
            for (int i = 0; i < (int)n.nprims; ++i) {
                const TriRec tr = tris[n.offset + i];
                float t, b1, b2;
                if (in && tri_intersect(o, d, mint, h.t, V3{tr.p1[0], tr.p1[1], tr.p1[2]},
                                        V3{tr.e1[0], tr.e1[1], tr.e1[2]}, V3{tr.e2[0], tr.e2[1], tr.e2[2]}, t, b1, b2)) {
                    h.t = t;
                    h.b1 = b1;
                    h.b2 = b2;
                    h.tri = tr.tri;
                }
            }
        }
        if (sp == 0) break;
        --sp;
        node = snode[sp];
        mask = __builtin_amdgcn_readfirstlane((uint32_t)smask[sp]) |
               ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(smask[sp] >> 32)) << 32);
    }
}

// trace_closest for every active lane, by sign packets: the lanes are grouped by their rays'
// direction signs and each group is traced as one packet (camera rays of one pixel share them).
// snode / smask: this wave's kTraceStack-entry stack in LDS.
__device__ Hit trace_closest_wave(const RenderScene &sc, V3 o, V3 d, float mint, float maxt, bool active, int *snode,
                                  uint64_t *smask) {
    Hit h;
    h.tri = INT_MIN;
    h.t = maxt;
    const V3 inv = V3{1.f / d.x, 1.f / d.y, 1.f / d.z};
    const int neg[3] = {inv.x < 0.f, inv.y < 0.f, inv.z < 0.f};
    const int sgn = neg[0] | (neg[1] << 1) | (neg[2] << 2);
    uint64_t todo = __builtin_amdgcn_ballot_w64(active);
    while (todo != 0) {
        const int lead = __builtin_ctzll(todo);
        const int pat = __builtin_amdgcn_readlane(sgn, lead);
        const uint64_t grp = __builtin_amdgcn_ballot_w64(active && sgn == pat) & todo;
        todo &= ~grp;
        trace_closest_packet(sc, o, inv, neg, d, mint, h, grp, pat, snode, smask);
    }
    if (active)
        for (int l = 0; l < sc.nlights; ++l) {
            if (sc.lights[l].kind) continue;  // an infinite light has no shape
            float t;
            V3 nn;
            if (sphere_hit_ool(sc.lights[l].s, o, d, mint, h.t, t, &nn)) {
                h.t = t;
                h.tri = -1 - l;
                h.lnn = nn;
            }
        }
    return h;
}

// Scene::IntersectP (bvh.cpp:442-488 + Sphere::IntersectP) for every active lane, as trace_any,
// by a stackless walk of the threaded BVH: pre-order, so after an interior node the walk goes on at
// node + 1 when some lane hit its box and at its subtree's end (the threaded offset) otherwise. A
// lane evaluates a node when node >= its resume index; missing a box sets resume to the subtree's
// end, a hit ends the lane. Each lane tests exactly the nodes and triangles its own traversal
// reaches with the fixed maxt (any-hit prunes only by the box test, so the order does not change
// the answer). strict: a triangle counts only when t < maxt (the BSDF ray toward an area light,
// whose own surface is at maxt). spheres: test the area-light spheres first, as trace_any does.
__device__ bool trace_any_wave(const RenderScene &sc, V3 o, V3 d, float mint, float maxt, bool active, bool strict,
                               bool spheres) {
    bool hit = false;
    if (active && spheres)
        for (int l = 0; l < sc.nlights; ++l) {
            float t;
            if (!sc.lights[l].kind && sphere_hit_ool(sc.lights[l].s, o, d, mint, maxt, t, nullptr)) {
                hit = true;
                break;
            }
        }
    const V3 inv = V3{1.f / d.x, 1.f / d.y, 1.f / d.z};
    const int neg[3] = {inv.x < 0.f, inv.y < 0.f, inv.z < 0.f};
    int resume = (active && !hit) ? 0 : INT_MAX;
    const cptr<BvhNode> nodes = as_const(sc.bvh_thread);
    const cptr<TriRec> tris = as_const(sc.tris);
    int node = 0;
    while (node < sc.nbvh) {
        node = __builtin_amdgcn_readfirstlane(node);
        const BvhNode n = nodes[node];
        const bool act = node >= resume;
        const bool in = act && bbox_hit(n, o, inv, neg, mint, maxt);
        if (act && !in) resume = n.nprims > 0 ? node + 1 : n.offset;
        if (n.nprims > 0) {
            if (__builtin_amdgcn_ballot_w64(in) != 0) {
                bool found = false;
                for (int i = 0; i < (int)n.nprims; ++i) {
                    const TriRec tr = tris[n.offset + i];
                    float t, b1, b2;
                    if (in && !found &&
                        tri_intersect(o, d, mint, maxt, V3{tr.p1[0], tr.p1[1], tr.p1[2]},
                                      V3{tr.e1[0], tr.e1[1], tr.e1[2]}, V3{tr.e2[0], tr.e2[1], tr.e2[2]}, t, b1, b2))
                        found = !strict || t < maxt;
                }
                if (found) {
                    hit = true;
                    resume = INT_MAX;
                }
                if (__builtin_amdgcn_ballot_w64(resume != INT_MAX) == 0) break;  // every lane is done
            }
            node = node + 1;
        } else {
            node = __builtin_amdgcn_ballot_w64(in) != 0 ? node + 1 : n.offset;
        }
    }
    return hit;
}
}  // namespace

}  // namespace mpss
