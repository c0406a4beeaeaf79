// profile_gpu.hip -- the LayeredSkin multipole profile built on the GPU.
//
// Same computation as material.cpp::channel_profile (MultipoleProfileTask::Run,
// multipole.cpp:241-295 -> MPC_ComputeDiffusionProfile, MultipoleProfileCalculator.cpp:151-346 ->
// MPC_ResampleForUniformDistanceSquaredDistribution :404-426), all 30 channels at once:
//   grid_fill_kernel   the dipole sums of both layers' R and T on the (i <= j) grid octant,
//                      lerp-on-thin-slab, written to the 8 symmetric cells of a 2M x 2M (M = 2N)
//                      zero-padded, origin-centred complex array (ToFrequencyDomain's layout)
//   fft_rows / fft_cols radix-2 FP64 FFTs in LDS (one row, or 4 columns, per workgroup)
//   combine_kernel     R12 = T1 R2 T1 / (1 - R2 R1) + R1 per frequency (CombineLayerProfiles)
//   readout_kernel     unique d^2 = (i^2 + j^2) step^2 samples, first (i, j) in the reference's
//                      loop order wins (:316-330)
//   total_kernel       Kahan sum of the R12 grid (totalReflectance)
//   resample_kernel    uniform-d^2 resampling to twice the sample count (:355-426)
// mc_reference_batch_gpu runs the same stages for the Monte-Carlo renderers' multipole references
// (MultipoleReferenceTask::Run, renderers/mcprofile.cpp:381-425): the combine also writes T12, both
// grids come back to the time domain, and ring_resample_kernel reads them at the ring centres.
// FP64 throughout the grids and transforms, like the reference's MPC; results agree with the
// host build (and the kissfft-based oracle) to FP64 rounding of differently ordered FFTs.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "material.h"

namespace mpss {

constexpr int kPairs = 11;  // dipole pairs -5..5 (DipoleCalculator)

struct DipoleP {
    float d, zpos, zneg, str, alphap;
};
struct ChanSetup {  // (named in material.h: GridWork holds an array of these)
    float s2;          // step^2 (float)
    double nf;         // step^2 as double
    double lerp[2];    // lerp-on-thin-slab weight per layer
    DipoleP dip[2][kPairs];
};

namespace {

constexpr float kPiMPC = 3.141592654f;  // numutil.h:45

float fresnel_diffuse_h(float eta) {  // DipoleCalculator.cpp:38-46
    if (eta >= 1.f) return -1.4399f / (eta * eta) + 0.7099f / eta + 0.6681f + 0.0636f * eta;
    const float e2 = eta * eta;
    return -0.4399f + 0.7099f / eta - 0.3319f / e2 + 0.0636f / (e2 * eta);
}

DipoleP make_dipole(float eta0, float etad, float thick, float sa, float sps, int zi, bool lerp) {
    DipoleP p;
    p.d = thick;
    const float spt = sa + sps;
    p.str = sqrtf(3 * sa * spt);
    p.alphap = sps / spt;
    const float F0 = fresnel_diffuse_h(eta0), Fd = fresnel_diffuse_h(etad);
    const float A0 = (1.f + F0) / (1.f - F0), Ad = (1.f + Fd) / (1.f - Fd);
    const float D = 1.f / (3.f * spt);
    const float zb0 = 2.f * A0 * D, zbd = 2.f * Ad * D;
    float l = 1.f / spt;
    if (lerp && l > p.d * .5f) l = p.d * .5f;
    p.zpos = 2.f * (float)zi * (p.d + zb0 + zbd) + l;
    p.zneg = p.zpos - 2.f * (l + zb0);
    return p;
}

__device__ __forceinline__ float dterm(float str, float z, float dsq) {
    const float r = sqrtf(dsq + z * z);
    return z * (1 + str * r) * expf(-str * r) / (r * r * r);
}

// grids: [nch][4][M * M] double2, 0 = R layer 0, 1 = T layer 0, 2 = R layer 1, 3 = T layer 1
__global__ void grid_fill_kernel(const ChanSetup *__restrict__ cs, int nch, int ext, int M, double2 *grids) {
    const int64_t per = (int64_t)(ext + 1) * (ext + 1);
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= per * 2 * nch) return;
    const int ch = (int)(gid / (per * 2)), l = (int)((gid / per) % 2);
    const int i = (int)((gid % per) / (ext + 1)), j = (int)(gid % (ext + 1));
    if (j < i) return;
    const ChanSetup &s = cs[ch];
    const double r2 = ((double)((unsigned)i * (unsigned)i) + (double)((unsigned)j * (unsigned)j)) * s.s2;
    const float r2f = (float)r2;
    double rr = 0., tt = 0.;
    for (int k = 0; k < kPairs; ++k) {
        const DipoleP &p = s.dip[l][k];
        const float rd = p.alphap * (0.25f / kPiMPC) * (dterm(p.str, p.zpos, r2f) - dterm(p.str, p.zneg, r2f));
        const float td = p.alphap * (0.25f / kPiMPC) * (dterm(p.str, p.d - p.zpos, r2f) - dterm(p.str, p.d - p.zneg, r2f));
        rr += rd * s.nf;
        tt += td * s.nf;
    }
    const double lerp = s.lerp[l];
    if (lerp < 1.) {
        rr *= lerp;
        tt *= lerp;
        if (i == 0 && j == 0) tt += 1. - lerp;
    }
    double2 *R = grids + ((size_t)ch * 4 + 2 * l) * (size_t)M * M;
    double2 *T = R + (size_t)M * M;
    const int ri[2] = {i, (M - i) % M}, rj[2] = {j, (M - j) % M};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            R[(size_t)ri[a] * M + rj[b]] = make_double2(rr, 0.);
            T[(size_t)ri[a] * M + rj[b]] = make_double2(tt, 0.);
            R[(size_t)rj[b] * M + ri[a]] = make_double2(rr, 0.);
            T[(size_t)rj[b] * M + ri[a]] = make_double2(tt, 0.);
        }
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cdiv(double2 a, double2 b) {
    const double den = b.x * b.x + b.y * b.y;
    return make_double2((a.x * b.x + a.y * b.y) / den, (a.y * b.x - a.x * b.y) / den);
}

// Iterative radix-2 DIT FFT of n points in LDS (bit-reversed load), 256 threads.
__device__ void lds_fft(double2 *a, int n, int logn, const double2 *__restrict__ tw, bool inverse) {
    for (int len = 2, st = n / 2; len <= n; len <<= 1, st >>= 1) {
        const int half = len >> 1;
        for (int b = threadIdx.x; b < n / 2; b += blockDim.x) {
            const int grp = b / half, k = b % half;
            const int i0 = grp * len + k, i1 = i0 + half;
            double2 w = tw[(size_t)k * st];
            if (inverse) w.y = -w.y;
            const double2 u = a[i0], v = cmul(a[i1], w);
            a[i0] = cadd(u, v);
            a[i1] = csub(u, v);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int bitrev(int x, int logn) { return (int)(__builtin_bitreverse32((unsigned)x) >> (32 - logn)); }

// one row per workgroup; blockIdx.y picks a block of rows mat_stride elements apart (the folded inverse
// transform of every channel's slot-0 grid)
__global__ __launch_bounds__(256) void fft_rows_kernel(double2 *data, int M, int logM, const double2 *tw, int inverse,
                                                       size_t mat_stride) {
    extern __shared__ double2 a_row[];
    double2 *row = data + (size_t)blockIdx.y * mat_stride + (size_t)blockIdx.x * M;
    for (int k = threadIdx.x; k < M; k += blockDim.x) a_row[bitrev(k, logM)] = row[k];
    __syncthreads();
    lds_fft(a_row, M, logM, tw, inverse != 0);
    for (int k = threadIdx.x; k < M; k += blockDim.x) row[k] = a_row[k];
}

// 'cols' adjacent columns per workgroup; grid = (M / cols) x nmat, matrices mat_stride elements apart
__global__ __launch_bounds__(256) void fft_cols_kernel(double2 *data, int M, int logM, int cols, const double2 *tw,
                                                       int inverse, size_t mat_stride) {
    extern __shared__ double2 a_col[];
    double2 *mat = data + (size_t)blockIdx.y * mat_stride;
    const int c0 = blockIdx.x * cols;
    for (int e = threadIdx.x; e < M * cols; e += blockDim.x) {
        const int r = e / cols, cc = e % cols;
        a_col[cc * M + bitrev(r, logM)] = mat[(size_t)r * M + c0 + cc];
    }
    __syncthreads();
    for (int cc = 0; cc < cols; ++cc) lds_fft(a_col + cc * M, M, logM, tw, inverse != 0);
    for (int e = threadIdx.x; e < M * cols; e += blockDim.x) {
        const int r = e / cols, cc = e % cols;
        mat[(size_t)r * M + c0 + cc] = a_col[cc * M + r];
    }
}

// R12 into slot 0 of each channel (CombineLayerProfiles, MultipoleProfileCalculator.cpp:253-280);
// with_t: also T12 = T1 T2 / (1 - R2 R1) into slot 1
__global__ void combine_kernel(double2 *grids, int nch, int M, int with_t) {
    const int64_t mm = (int64_t)M * M;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= mm * nch) return;
    const int ch = (int)(gid / mm);
    const int64_t k = gid % mm;
    double2 *g = grids + (size_t)ch * 4 * mm;
    const double2 fR1 = g[k], fT1 = g[mm + k], fR2 = g[2 * mm + k];
    const double2 one = csub(make_double2(1., 0.), cmul(fR2, fR1));
    g[k] = cadd(cdiv(cmul(cmul(fT1, fR2), fT1), one), fR1);
    if (with_t) g[mm + k] = cdiv(cmul(fT1, g[3 * mm + k]), one);
}

// unique d^2 entries: value = Re(R12)(i, j) / M^2 as float * 1 / step^2
__global__ void readout_kernel(const double2 *grids, int nch, int M, const int2 *ij, const uint32_t *nsq, int nent,
                               const float *step, float *d_out, float *r_out) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nent * nch) return;
    const int ch = gid / nent, k = gid % nent;
    const double2 *R = grids + (size_t)ch * 4 * M * M;
    const double s = 1.0 / ((double)M * (double)M);
    const float st = step[ch];
    const float denorm = 1.f / (st * st);
    const int2 p = ij[k];
    r_out[gid] = (float)(R[(size_t)p.x * M + p.y].x * s) * denorm;
    d_out[gid] = (float)nsq[k] * st * st;
}

// totalReflectance = Kahan sum over the N x N time-domain grid (numutil.h:236-246), per channel; slot 1 holds
// T12 where the combine wrote it (totalTransmittance). out[ch * out_stride]
__global__ __launch_bounds__(256) void total_kernel(const double2 *grids, int M, int N, int slot, double *out,
                                                    int out_stride) {
    __shared__ double part[256];
    const int ch = blockIdx.x;
    const double2 *R = grids + ((size_t)ch * 4 + slot) * M * M;
    const double s = 1.0 / ((double)M * (double)M);
    const int c = (N - 1) / 2;
    double sum = 0., comp = 0.;
    for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
        const int i = e / N, j = e % N;
        const double x = R[(size_t)((M - c + i) % M) * M + (M - c + j) % M].x * s;
        const double y = x - comp, t = sum + y;
        comp = (t - sum) - y;
        sum = t;
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0., cp = 0.;
        for (int k = 0; k < (int)blockDim.x; ++k) {
            const double y = part[k] - cp, t = tot + y;
            cp = (t - tot) - y;
            tot = t;
        }
        out[(size_t)ch * out_stride] = tot;
    }
}

// MPC resample at one d^2 (MultipoleProfileCalculator.cpp:355-402)
__device__ float resample_dev(const float *d, const float *R, unsigned len, float dsq) {
    if (dsq > d[len - 1]) return 0.f;
    unsigned lo = 0, hi = len - 1;
    float d2lo = d[lo];
    if (lo + 32 < hi) {
        float d2hi = d[hi];
        do {
            int m = (int)((dsq - d2lo) / (d2hi - d2lo) * (float)(hi - lo));
            m = m < 0 ? 0 : (m > (int)(hi - lo - 1) ? (int)(hi - lo - 1) : m);
            const unsigned mid = (unsigned)m + lo;
            const float d2mid = d[mid];
            if (dsq > d2mid) {
                lo = mid + 1;
                d2lo = d[lo];
            } else {
                hi = mid;
                d2hi = d2mid;
            }
        } while (lo + 32 < hi);
    }
    while (lo < hi && dsq > d2lo) d2lo = d[++lo];
    if (!lo) return R[0];
    float t = (dsq - d[lo - 1]) / (d[lo] - d[lo - 1]);
    t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
    if (t != t) t = 0.5f;
    return (1.f - t) * R[lo - 1] + t * R[lo];
}

__global__ void resample_kernel(const float *d, const float *r, int nent, int nch, int tl, float *table) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= tl * nch) return;
    const int ch = gid / tl, i = gid % tl;
    const float *dc = d + (size_t)ch * nent, *rc = r + (size_t)ch * nent;
    const float extent = dc[nent - 1];
    const float q = (float)i * extent / (float)(tl - 1);
    table[gid] = resample_dev(dc, rc, (unsigned)nent, q);
}

// first (i, j) per unique i^2 + j^2 in the reference's loop order (i ascending, j >= i), sorted by
// nsq -- depends only on ext, so it is built once per length
struct UniqueList {
    std::vector<int2> ij;
    std::vector<uint32_t> nsq;
};
const UniqueList &unique_list(unsigned ext) {
    static std::mutex mu;
    static std::map<unsigned, UniqueList> cache;
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(ext);
    if (it != cache.end()) return it->second;
    std::vector<uint8_t> seen((size_t)ext * ext * 2 + 1, 0);
    std::vector<std::pair<uint32_t, int2>> ents;
    for (unsigned i = 0; i <= ext; ++i)
        for (unsigned j = i; i * i + j * j <= ext * ext; ++j) {
            const unsigned n = i * i + j * j;
            if (seen[n]) continue;
            seen[n] = 1;
            ents.emplace_back(n, make_int2((int)i, (int)j));
        }
    std::sort(ents.begin(), ents.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    UniqueList &u = cache[ext];
    for (auto &e : ents) {
        u.nsq.push_back(e.first);
        u.ij.push_back(e.second);
    }
    return u;
}

// the grid fill's constants for two layers at a given step (layer_grid, material.cpp; the Fresnel ratios
// as MPC_ComputeDiffusionProfile passes them, :294-314)
void two_layer_setup(const MpcLayer L[2], float step, bool lerp_thin, ChanSetup &c) {
    c.s2 = step * step;
    c.nf = c.s2;
    const float up[2] = {L[0].ior, L[1].ior / L[0].ior}, lo[2] = {L[0].ior / L[1].ior, L[1].ior};
    for (int l = 0; l < 2; ++l) {
        float thick = L[l].thickness;
        const float mua = L[l].mua, musp = L[l].musp;
        const double mfp2 = 2. / (mua + musp);
        double lerp = 1.;
        if (lerp_thin) {
            lerp = (thick < mfp2) ? (1. - exp(-thick * 2. / mfp2)) / (1. - exp(-2.)) : 1.;
            if (thick < 0.01 * mfp2) thick = (float)(0.01 * mfp2);
        }
        c.lerp[l] = lerp;
        for (int k = 0; k < kPairs; ++k) c.dip[l][k] = make_dipole(up[l], lo[l], thick, mua, musp, k - 5, lerp_thin);
    }
}

// per-channel setup (channel_profile / layer_grid, material.cpp); returns the channel's step
float chan_setup(const LayerParams &lp, int sc, int desired_length, bool lerp_thin, ChanSetup &c) {
    float mfp_total = 0.f;
    for (int l = 0; l < 2; ++l) mfp_total += 1.f / (lp.mua[l][sc] + lp.musp[l][sc]);
    const float mfp = mfp_total / (float)2;
    const float step = 12.f * mfp / (float)desired_length;
    const MpcLayer L[2] = {{lp.mua[0][sc], lp.musp[0][sc], lp.eta[0], lp.thickness[0]},
                           {lp.mua[1][sc], lp.musp[1][sc], lp.eta[1], lp.thickness[1]}};
    two_layer_setup(L, step, lerp_thin, c);
    return step;
}

// the fit's resampling (GaussianFitTask::Run, profilefit.cpp:191): as many entries as the profile has
// samples, and both arrays kept -- d^2 as MPC_ResampleForUniformDistanceSquaredDistribution writes it
__global__ void resample_fit_kernel(const float *d, const float *r, int nent, int nch, float *dsq_out, float *r_out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)nent * nch) return;
    const int ch = (int)(gid / nent), i = (int)(gid % nent);
    const float *dc = d + (size_t)ch * nent, *rc = r + (size_t)ch * nent;
    const float extent = dc[nent - 1];
    const float q = (float)i * extent / (float)(nent - 1);
    dsq_out[gid] = q;
    r_out[gid] = resample_dev(dc, rc, (unsigned)nent, q);
}

// MPC_ResampleDistribution (MultipoleProfileCalculator.cpp:429-449) at the MC profile's ring centres
// (MultipoleReferenceTask::Run, mcprofile.cpp:405-413): point = (float)((i + .5) * (extent / nseg)),
// d^2 = point * point in float; R and T of slab ch into out_r / out_t [nch][nseg] as doubles
__global__ void ring_resample_kernel(const float *d, const float *r, const float *t, int nent, int nch,
                                     const double *extent, int nseg, double *out_r, double *out_t) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)nseg * nch) return;
    const int ch = (int)(gid / nseg), i = (int)(gid % nseg);
    const float *dc = d + (size_t)ch * nent;
    const float point = (float)((i + .5) * (extent[ch] / nseg));
    const float dsq = point * point;
    out_r[gid] = resample_dev(dc, r + (size_t)ch * nent, (unsigned)nent, dsq);
    out_t[gid] = resample_dev(dc, t + (size_t)ch * nent, (unsigned)nent, dsq);
}

unsigned round_up_pow2_u(unsigned v) {
    v--;
    v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    return v + 1;
}

// ---- the grid pipeline: one plan, one workspace, one launch sequence for the three drivers below

// Sizes for n_channels channels at desired_length; the batch is what grid_budget_bytes of grids hold, the
// caller's cap (max_batch > 0) and the launch grids' limit (grid.y = 4 nch <= 65535) allow.
GridPlan make_grid_plan(int desired_length, int n_channels, int max_batch, size_t grid_budget_bytes) {
    if (n_channels < 1) throw Error(-1, "multipole grids: no channels");
    GridPlan p;
    p.length = (int)round_up_pow2_u((unsigned)desired_length);
    p.N = 2 * p.length;
    p.M = 2 * p.N;
    p.logM = 0;
    while ((1 << p.logM) < p.M) ++p.logM;
    if (desired_length < 2 || p.M > 4096) throw Error(-1, "multipole grids: desired length outside 2..1024");
    p.ext = p.length - 1;
    p.nent = (int)unique_list((unsigned)p.ext).nsq.size();
    p.cols = std::max(1, std::min(4, 131072 / (p.M * (int)sizeof(double2))));
    const size_t grid_bytes = (size_t)p.M * p.M * sizeof(double2);
    size_t batch = std::max<size_t>(1, grid_budget_bytes / (4 * grid_bytes));
    batch = std::min<size_t>(batch, 16383);
    if (max_batch > 0) batch = std::min<size_t>(batch, (size_t)max_batch);
    p.batch = (int)std::min<size_t>(batch, (size_t)n_channels);
    return p;
}

// twiddles exp(-2 pi i k / M)
std::vector<double2> make_twiddles(int M) {
    std::vector<double2> tw(M / 2);
    for (int k = 0; k < M / 2; ++k) {
        const double ph = -2.0 * M_PI * (double)k / (double)M;
        tw[k] = make_double2(cos(ph), sin(ph));
    }
    return tw;
}

// Every allocation and every (blocking) upload of the pipeline for the channels cs / steps, and the kernels'
// dynamic-LDS limits, which have to be raised before the first launch at this M: at M = 4096 the rows
// kernel needs 64 KB and the columns kernel 128 KB.
void grid_prepare(const GridPlan &p, const std::vector<ChanSetup> &cs, const std::vector<float> &steps, bool with_t,
                  GridWork &w) {
    const UniqueList &ul = unique_list((unsigned)p.ext);
    const std::vector<double2> tw = make_twiddles(p.M);
    w.plan = p;
    w.n = (int)cs.size();
    w.batches = 0;
    w.tw.upload(tw.data(), tw.size());
    w.setup.upload(cs.data(), cs.size());
    w.ij.upload(ul.ij.data(), ul.ij.size());
    w.nsq.upload(ul.nsq.data(), ul.nsq.size());
    w.step.upload(steps.data(), steps.size());
    w.d.alloc((size_t)p.batch * p.nent);
    w.r.alloc((size_t)p.batch * p.nent);
    if (with_t) w.t.alloc((size_t)p.batch * p.nent);
    w.grids.alloc((size_t)p.batch * 4 * p.M * p.M);
    MPSS_HIP(hipFuncSetAttribute((const void *)fft_cols_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 p.cols * p.M * (int)sizeof(double2)));
    MPSS_HIP(hipFuncSetAttribute((const void *)fft_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 p.M * (int)sizeof(double2)));
}

// One batch, channels c0 .. c0 + nch - 1 (nch <= the plan's batch): their time-domain R12 is left in slot 0
// of w.grids (T12 in slot 1 when with_t) and its unique-d^2 samples in w.d / w.r (w.t) [nch][nent].
// A memset and kernels on `stream` only: nothing is allocated, copied from the host or waited for.
void grid_launch(GridWork &w, int c0, int nch, bool with_t, hipStream_t stream) {
    const GridPlan &p = w.plan;
    if (nch < 1 || nch > p.batch || c0 < 0 || c0 + nch > w.n || (with_t && !w.t.ptr))
        throw Error(-1, "multipole grids: range outside the prepared work");
    const int M = p.M, logM = p.logM, cols = p.cols, nent = p.nent;
    const size_t mm = (size_t)M * M, chan_stride = 4 * mm, row_lds = M * sizeof(double2), col_lds = cols * row_lds;
    double2 *g = w.grids.ptr;
    MPSS_HIP(hipMemsetAsync(g, 0, (size_t)nch * chan_stride * sizeof(double2), stream));
    const int64_t cells = (int64_t)(p.ext + 1) * (p.ext + 1) * 2 * nch;
    hipLaunchKernelGGL(grid_fill_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, w.setup.ptr + c0,
                       nch, p.ext, M, g);
    // forward 2-D transforms of all 4 grids
    hipLaunchKernelGGL(fft_rows_kernel, dim3((unsigned)(M * 4), (unsigned)nch), dim3(256), row_lds, stream, g, M, logM,
                       w.tw.ptr, 0, chan_stride);
    hipLaunchKernelGGL(fft_cols_kernel, dim3((unsigned)(M / cols), (unsigned)(nch * 4)), dim3(256), col_lds, stream, g,
                       M, logM, cols, w.tw.ptr, 0, mm);
    const int64_t freq = (int64_t)mm * nch;
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((freq + 255) / 256)), dim3(256), 0, stream, g, nch, M,
                       with_t ? 1 : 0);
    // inverse transforms of every channel's R12 (slot 0) and T12 (slot 1, with_t), folded over the channels:
    // the two slots are adjacent, so one rows launch covers both; the columns go slot by slot
    const int slots = with_t ? 2 : 1;
    hipLaunchKernelGGL(fft_rows_kernel, dim3((unsigned)(M * slots), (unsigned)nch), dim3(256), row_lds, stream, g, M,
                       logM, w.tw.ptr, 1, chan_stride);
    for (int slot = 0; slot < slots; ++slot)
        hipLaunchKernelGGL(fft_cols_kernel, dim3((unsigned)(M / cols), (unsigned)nch), dim3(256), col_lds, stream,
                           g + slot * mm, M, logM, cols, w.tw.ptr, 1, chan_stride);
    // the readout takes a channel's grid at grids + ch * 4 M^2: offset by one grid it reads T12
    float *const out[2] = {w.r.ptr, w.t.ptr};
    const unsigned rb = (unsigned)(((int64_t)nent * nch + 255) / 256);
    for (int slot = 0; slot < slots; ++slot)
        hipLaunchKernelGGL(readout_kernel, dim3(rb), dim3(256), 0, stream, g + slot * mm, nch, M, w.ij.ptr, w.nsq.ptr,
                           nent, w.step.ptr + c0, w.d.ptr, out[slot]);
    MPSS_HIP(hipGetLastError());
    ++w.batches;
}

}  // namespace

void build_profile_gpu(const LayerParams &lp, int desired_length, bool lerp_thin, ProfileTables &out,
                       hipStream_t stream, int distinct) {
    if (distinct < 1 || distinct > NB) throw Error(-1, "build_profile_gpu: distinct channels out of range");
    const int NC = distinct;  // channels built; channel c >= NC copies channel c % NC
    // 3 GB of grids at most, so that a render context's peak memory stays where it was
    const GridPlan p = make_grid_plan(desired_length, NC, 0, (size_t)3 << 30);
    const int nent = p.nent, tl = 2 * nent;
    std::vector<ChanSetup> cs(NC);
    std::vector<float> steps(NC);
    for (int sc = 0; sc < NC; ++sc) steps[sc] = chan_setup(lp, sc, desired_length, lerp_thin, cs[sc]);
    GridWork w;
    grid_prepare(p, cs, steps, false, w);
    DevBuf<float> d_table;
    d_table.alloc((size_t)NC * tl);
    DevBuf<double> d_tot;
    d_tot.alloc(NC);
    std::vector<float> dlast(NC);
    for (int c0 = 0; c0 < NC; c0 += p.batch) {
        const int nch = std::min(p.batch, NC - c0);
        grid_launch(w, c0, nch, false, stream);
        hipLaunchKernelGGL(total_kernel, dim3((unsigned)nch), dim3(256), 0, stream, w.grids.ptr, p.M, p.N, 0,
                           d_tot.ptr + c0, 1);
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((tl * nch + 255) / 256)), dim3(256), 0, stream, w.d.ptr,
                           w.r.ptr, nent, nch, tl, d_table.ptr + (size_t)c0 * tl);
        MPSS_HIP(hipGetLastError());
        for (int c = 0; c < nch; ++c)  // the channel's extent, before the next batch overwrites w.d
            MPSS_HIP(hipMemcpyAsync(&dlast[c0 + c], w.d.ptr + (size_t)c * nent + nent - 1, sizeof(float),
                                    hipMemcpyDeviceToHost, stream));
    }
    out.length = tl;
    out.table.resize((size_t)NB * tl);
    std::vector<double> tot(NC);
    MPSS_HIP(hipMemcpyAsync(out.table.data(), d_table.ptr, sizeof(float) * (size_t)NC * tl, hipMemcpyDeviceToHost,
                            stream));
    MPSS_HIP(hipMemcpyAsync(tot.data(), d_tot.ptr, sizeof(double) * NC, hipMemcpyDeviceToHost, stream));
    MPSS_HIP(hipStreamSynchronize(stream));
    for (int c = NC; c < NB; ++c)
        memcpy(&out.table[(size_t)c * tl], &out.table[(size_t)(c % NC) * tl], sizeof(float) * tl);
    for (int c = 0; c < NB; ++c) {
        const float extent = dlast[c % NC];
        const float last = (float)(tl - 1) * extent / (float)(tl - 1);
        out.spacing[c] = last / (float)(tl - 1);  // multipole.cpp:274-275
        out.rcp[c] = (float)(tl - 1) / last;
        out.total_reflectance[c] = (float)tot[c % NC];
    }
}

// GaussianFitTask::Run's profiles (profilefit.cpp:158-192) for n channels: the grid pipeline with the thin-slab
// lerp on, then the fit's resampling.
int fit_profiles_prepare(const LayerParams *lp, int n, int desired_length, int max_batch, GridWork &w) {
    const GridPlan p = make_grid_plan(desired_length, n, max_batch, (size_t)8 << 30);
    std::vector<ChanSetup> cs((size_t)n);
    std::vector<float> steps((size_t)n);
    for (int i = 0; i < n; ++i) steps[i] = chan_setup(lp[i / NB], i % NB, desired_length, true, cs[i]);
    grid_prepare(p, cs, steps, false, w);
    return p.batch;
}

void fit_profiles_launch(int c0, int nch, float *dsq_dev, float *refl_dev, GridWork &w, hipStream_t stream) {
    grid_launch(w, c0, nch, false, stream);
    const int nent = w.plan.nent;
    hipLaunchKernelGGL(resample_fit_kernel, dim3((unsigned)(((int64_t)nent * nch + 255) / 256)), dim3(256), 0, stream,
                       w.d.ptr, w.r.ptr, nent, nch, dsq_dev, refl_dev);
    MPSS_HIP(hipGetLastError());
}

// MultipoleReferenceTask::Run (renderers/mcprofile.cpp:381-425) for nslabs two-layer stacks: what
// mc_reference_profile (material.cpp) computes on the host. Beyond the fit's profile: the step is
// (float)(extent * 1.01 / desired_length), the combine writes T12 beside R12, both come back to the time
// domain, both are read out and Kahan-summed, and the profile is read at the ring centres. A slab's grids
// are its own, so its result does not depend on the batch size. One wait at the end.
void mc_reference_batch_gpu(const MpcLayer *layers, int nslabs, const double *extent, int nsegments,
                            int desired_length, bool lerp_thin, int max_batch, double *refl, double *trans,
                            double *total_r, double *total_t, hipStream_t stream) {
    // 8 GB of grids at most: 1 GiB per slab at M = 4096
    const GridPlan p = make_grid_plan(desired_length, nslabs, max_batch, (size_t)8 << 30);
    std::vector<ChanSetup> cs((size_t)nslabs);
    std::vector<float> steps((size_t)nslabs);
    for (int s = 0; s < nslabs; ++s) {
        steps[s] = (float)(extent[s] * 1.01 / desired_length);
        two_layer_setup(layers + 2 * (size_t)s, steps[s], lerp_thin, cs[s]);
    }
    GridWork w;
    grid_prepare(p, cs, steps, true, w);
    DevBuf<double> d_ext, d_out;  // d_out: rings R [nslabs][nseg], rings T, then totals [nslabs][2]
    d_ext.upload(extent, (size_t)nslabs);
    const size_t nring = (size_t)nslabs * nsegments;
    d_out.alloc(2 * nring + 2 * (size_t)nslabs);
    double *o_r = d_out.ptr, *o_t = o_r + nring, *o_tot = o_t + nring;
    for (int c0 = 0; c0 < nslabs; c0 += p.batch) {
        const int nch = std::min(p.batch, nslabs - c0);
        grid_launch(w, c0, nch, true, stream);
        for (int slot = 0; slot < 2; ++slot)
            hipLaunchKernelGGL(total_kernel, dim3((unsigned)nch), dim3(256), 0, stream, w.grids.ptr, p.M, p.N, slot,
                               o_tot + 2 * (size_t)c0 + slot, 2);
        hipLaunchKernelGGL(ring_resample_kernel, dim3((unsigned)(((int64_t)nsegments * nch + 255) / 256)), dim3(256), 0,
                           stream, w.d.ptr, w.r.ptr, w.t.ptr, p.nent, nch, d_ext.ptr + c0, nsegments,
                           o_r + (size_t)c0 * nsegments, o_t + (size_t)c0 * nsegments);
        MPSS_HIP(hipGetLastError());
    }
    std::vector<double> tot(2 * (size_t)nslabs);
    if (refl) MPSS_HIP(hipMemcpyAsync(refl, o_r, sizeof(double) * nring, hipMemcpyDeviceToHost, stream));
    if (trans) MPSS_HIP(hipMemcpyAsync(trans, o_t, sizeof(double) * nring, hipMemcpyDeviceToHost, stream));
    MPSS_HIP(hipMemcpyAsync(tot.data(), o_tot, sizeof(double) * tot.size(), hipMemcpyDeviceToHost, stream));
    MPSS_HIP(hipStreamSynchronize(stream));
    for (int s = 0; s < nslabs; ++s) {  // MPC_Output's totals are floats
        total_r[s] = (float)tot[2 * (size_t)s];
        total_t[s] = (float)tot[2 * (size_t)s + 1];
    }
}

}  // namespace mpss

