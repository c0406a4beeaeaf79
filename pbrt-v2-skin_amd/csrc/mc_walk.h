// mc_walk.h -- the per-event step of ProfileRendererTask::TraceSinglePhoton (reference
// src/renderers/mcprofile.cpp:229-341), device code shared by the single-slab kernel
// (mc_profile.hip) and the batched one (mc_profile_batch.hip): one copy of the walk arithmetic, so
// a slab traced in a batch follows the same photon paths as the slab traced alone.
#pragma once
#include "mc_profile.h"

namespace mpss {

constexpr int kMcMaxSegments = 4096;  // ComputeMonteCarloProfile tallies 4096 rings (multipole.cpp:322)
constexpr int kMcPool = 256;          // photon ids a wave takes from the global counter at a time
// pbrt's M_PI is the float literal 3.14159265358979323846f (core/pbrt.h:193-196); the walk and the
// ring normalisation use it widened to double
constexpr double kPbrtPi = (double)3.14159265358979323846f;

// UniformSampleSphereD (mcprofile.cpp:51-58); u1 is drawn before u2
__device__ __forceinline__ void sample_sphere_d(double u1, double u2, double &x, double &y, double &z) {
    z = 1. - 2. * u1;
    const double r = sqrt(fmax(0., 1. - z * z));
    const double phi = 2. * kPbrtPi * u2;
    double sp, cp;
    sincos(phi, &sp, &cp);  // one range reduction for both (the same values as cos / sin)
    x = r * cp;
    y = r * sp;
}

// FrDiel<double> (core/reflection.cpp:72-80) with etat = 1
__device__ __forceinline__ double fr_diel_d(double cosi, double cost, double etai, double etat) {
    const double rparl = ((etat * cosi) - (etai * cost)) / ((etat * cosi) + (etai * cost));
    const double rperp = ((etai * cosi) - (etat * cost)) / ((etai * cosi) + (etat * cost));
    return (rparl * rparl + rperp * rperp) / 2.;
}

struct McPhoton {  // one lane's photon between events
    double ox, oy, oz, dx, dy, dz;
    double thr, len, mfp;
    int layer;
    McRng rng;
};

// TraceSinglePhoton setup (:233-241), then the outer loop's head (:245-248)
__device__ __forceinline__ void mc_photon_start(const McScene &sc, uint64_t seed, uint64_t id, McPhoton &p) {
    p.rng.init(seed, id);
    p.ox = p.oy = p.oz = 0.;
    p.dx = p.dy = 0.;
    p.dz = 1.;
    p.thr = 1.;
    p.len = 0.;
    p.layer = 0;
    p.mfp = sc.mfp[0];
    p.len *= p.mfp;
}

// One event of a live photon: a free flight that ends in a scatter inside the layer or on an interface.
// tally(top, seg, weight) is called when the photon leaves through the top (reflectance) or the bottom
// (transmittance) inside the extent. Returns whether the photon is still alive.
template <class Tally>
__device__ __forceinline__ bool mc_walk_event(const McScene &sc, McPhoton &p, Tally &&tally) {
    double &ox = p.ox, &oy = p.oy, &oz = p.oz, &dx = p.dx, &dy = p.dy, &dz = p.dz;
    double &thr = p.thr, &len = p.len, &mfp = p.mfp;
    int &layer = p.layer;
    McRng &rng = p.rng;
    bool alive = true;
    const McLayer &L = sc.layer[layer];
    // free flight (:251-252)
    if (len == 0.) len = fmin(-log((double)1.f - rng.next()), 1e7) * mfp;
    // MiniScene::Intersect (:153-185) with maxt = len
    bool hit = false;
    int iface = 0;
    double t = 0., inv = 1.;
    const double ct = dz;
    if (ct != 0.) {
        if (dz > 0.) {
            const double nd = sc.depth[layer + 1];
            if (nd - oz < ct * len) {
                hit = true;
                iface = layer + 1;
                t = (nd - oz) / ct;
                inv = sc.eta_dn[layer];
            }
        } else {
            const double nd = sc.depth[layer];
            if (nd - oz > ct * len) {
                hit = true;
                iface = layer;
                t = (nd - oz) / ct;
                inv = sc.eta_up[layer];
            }
        }
    }
    // the step's attenuation: to the interface (a hit) or over the free flight (a scatter) --
    // one exp for the wave, whichever branch each lane takes
    double px = 0., py = 0., pz = 0., dist = 0.;
    if (hit) {
        px = ox + dx * t;
        py = oy + dy * t;
        pz = oz + dz * t;
        const double ex = px - ox, ey = py - oy, ez = pz - oz;
        dist = sqrt(ex * ex + ey * ey + ez * ez);
    }
    thr *= exp((double)-L.mua * (hit ? dist : len));
    if (hit) {
        len = fmax(1e-7 * mfp, len - dist);
        const double cosi = fmin(fmax(dz, -1.), 1.);
        const bool up = dz < 0.;
        const double sint2 = (1. - cosi * cosi) * inv * inv;
        double cost = 0.;
        bool reflect;
        if (sint2 >= 1.) {
            reflect = true;  // total internal reflection
        } else {
            cost = sqrt(fmax(0., 1. - sint2));
            const double F = fr_diel_d(fabs(cosi), cost, inv, 1.);
            reflect = rng.next() < F;
        }
        int target = layer;
        if (reflect) {
            dz = -dz;
        } else {
            target = up ? layer - 1 : layer + 1;
            dx = inv * dx;
            dy = inv * dy;
            dz = up ? -cost : cost;
        }
        ox = px;
        oy = py;
        oz = pz;
        if (target != layer) {
            // book-keeping (:303-316)
            if (iface == 0 || iface == sc.nlayers) {
                const double rd = sqrt(px * px + py * py + 0. * 0.);
                const int seg = (int)(rd * sc.nsegments / sc.extent);
                if (rd < sc.extent && seg < sc.nsegments) tally(iface == 0, seg, thr);
            }
            // outer loop tail (:330-340): roulette, then remaining length in the old layer's mfp units
            bool dead = false;
            if (thr < 1e-5) {
                const double q = thr * 1e5;
                if (rng.next() > q)
                    dead = true;
                else
                    thr /= q;
            }
            if (!dead) {
                len *= (double)L.musp;
                layer = target;
                if (layer < 0 || layer >= sc.nlayers) {
                    dead = true;
                } else {
                    mfp = sc.mfp[layer];  // next outer loop's head
                    len *= mfp;
                }
            }
            if (dead) alive = false;
        }
    } else {
        // scatter inside the layer (:319-327)
        ox = ox + dx * len;
        oy = oy + dy * len;
        oz = oz + dz * len;
        len = 0.;
        const double u1 = rng.next(), u2 = rng.next();
        sample_sphere_d(u1, u2, dx, dy, dz);
    }
    return alive;
}

}  // namespace mpss
