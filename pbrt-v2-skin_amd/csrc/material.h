// material.h -- LayeredSkin material preparation (host side).
//
// Follows the reference's parse-time precompute for `Material "layeredskin"`:
//   CreateLayeredSkinMaterial / LayeredSkin::LayeredSkin  (src/materials/layeredskin.cpp:39-123, 222-262)
//   SkinCoefficients                                       (src/materials/skincoeffs.h:38-158)
//   ComputeMultipoleProfile -> MultipoleProfileTask::Run   (src/core/multipole.cpp:241-295, 371-406)
//   MPC_ComputeDiffusionProfile + resample                 (MultipoleProfileCalculator.cpp:151-426)
//   ComputeRhoDataFromBxDF                                 (src/core/multipole.cpp:466-549)
// The product's Rd table is channel-major: table[c * length + k].
#pragma once
#include <vector>
#include "common.h"

namespace mpss {

struct SkinParams {
    float roughness = 0.4f, nmperunit = 100e6f;
    float f_mel = 0.15f, f_eu = 1.f, f_blood = 0.002f, f_ohg = 0.3f;
    float thickness_nm[2] = {0.25e6f, 20e6f};
    float ior[2] = {1.4f, 1.4f};
    int desired_length = 512;
    bool lerp_on_thin_slab = true;
    bool double_ref_sslf = false;
};

struct LayerParams {
    float mua[2][NB], musp[2][NB], thickness[2], eta[2];
};

struct ProfileTables {
    int length = 0;                   // entries per channel (resampled)
    std::vector<float> table;         // [NB][length]
    float rcp[NB], spacing[NB], total_reflectance[NB];
};

struct RhoTable {
    std::vector<float> hd;  // [n] scalar rho_hd(cos theta) (all channels equal for this BxDF)
    float hh = 0.f;
};

void skin_layer_params(const SkinParams &p, LayerParams &out);
// Renderer "multipoleprofilefit" (renderers/profilefit.cpp): a combination's layers in millimetres
// (CreateGaussianFitTasks :262-274), the mfp range the sigma list is made from (DoProfileFit :287-300,
// folded into mfp_min / mfp_max), and one channel's profile as the fit reads it (GaussianFitTask::Run
// :158-192: d^2 and R resampled to the sample count itself)
void skin_fit_layer_params(float f_mel, float f_eu, float f_blood, float f_ohg, const float thickness_nm[2],
                           const float ior[2], LayerParams &out);
void skin_fit_mfp_range(float f_mel, float f_eu, float f_blood, float f_ohg, float &mfp_min, float &mfp_max);
void fit_channel_profile(const LayerParams &lp, int sc, int desired_length, std::vector<float> &dsq,
                         std::vector<float> &refl);
// The grid pipeline of the GPU multipole builders (profile_gpu.hip): every channel takes four M x M complex
// FP64 transform grids, and the channels go through them `batch` at a time.
struct GridPlan {
    int length, N, M, logM, ext;  // desired_length rounded up to a power of two, N = 2 length, M = 2 N, ext = length - 1
    int nent, cols, batch;  // a profile's unique d^2 samples; columns per workgroup of the column transform; batch size
};
struct ChanSetup;  // the grid fill's constants of one channel (profile_gpu.hip)
// The pipeline's device workspace. It must outlive the work queued on the stream: the fit path returns from
// its launches with the work still queued (the caller's hipStreamSynchronize ends it); build_profile_gpu and
// mc_reference_batch_gpu synchronise before they return.
struct GridWork {
    GridPlan plan;
    DevBuf<double2> grids, tw;
    DevBuf<ChanSetup> setup;  // [n]
    DevBuf<int2> ij;
    DevBuf<uint32_t> nsq;
    DevBuf<float> step;     // [n]
    DevBuf<float> d, r, t;  // a batch's unique-d^2 samples [batch][nent]; t only where T12 is wanted
    int n = 0;              // channels prepared
    int batches = 0;        // batches launched so far
};
// fit_channel_profile for n channels on the current HIP device: lp[i / NB] band i % NB is channel i, in
// batches of at most max_batch (0: as many as 8 GB of grids hold); a channel's result does not depend on the
// split. fit_profiles_prepare does every allocation and (blocking) host copy and returns the batch size;
// fit_profiles_launch queues one batch (channels c0 .. c0 + nch - 1, nch <= the batch size) on `stream` -- a
// memset and kernels only -- and writes its d^2 and R to dsq_dev / refl_dev [nch][work.plan.nent].
int fit_profiles_prepare(const LayerParams *lp, int n, int desired_length, int max_batch, GridWork &work);
void fit_profiles_launch(int c0, int nch, float *dsq_dev, float *refl_dev, GridWork &work, hipStream_t stream);
// distinct: channels 0..distinct-1 are built and channel c >= distinct copies channel c % distinct
// (rgbprofile: lp's band c already holds component c % 3, so 3 builds give all 30 rows)
void build_profile(const LayerParams &lp, int desired_length, bool lerp_on_thin_slab, ProfileTables &out,
                   int nthreads = 0, int distinct = NB);
// The same profile built on the current HIP device (profile_gpu.hip); out is filled on the host.
void build_profile_gpu(const LayerParams &lp, int desired_length, bool lerp_on_thin_slab, ProfileTables &out,
                       hipStream_t stream = 0, int distinct = NB);
// The same rho_hd table on the current HIP device (rho_gpu.hip): bit-identical to build_rho_table
// (one MT19937 stream per entry, terms Kahan-summed in sample order); rho_hh on the host.
void build_rho_table_gpu(float roughness, float eta, bool fixed_fresnel, int n_entries, int sqrt_samples,
                         RhoTable &out, hipStream_t stream = 0);
// ComputeRhoHHFromBxDF (multipole.cpp:466-480)
float rho_hh(float roughness, float eta, bool fixed_fresnel, int sqrt_samples);
// LayeredSkin "showirradiancepoints": ComputeIrradiancePointsProfile(radius) (multipole.cpp:551-567) --
// every band the two-entry table {1 / area, 1 / area}, area = (float)(M_PI * r * r), dsqSpacing = r * r,
// so Rd(d^2) = 1 / area for d < r and 0 beyond -- and ComputeRoughRhoData (:569-572): rho_hd = {0, 0}.
void irradiance_points_profile(float radius, ProfileTables &p, RhoTable &rho);
void build_rho_table(float roughness, float eta, bool fixed_fresnel, int n_entries, int sqrt_samples,
                     RhoTable &out, int nthreads = 0);

// MPC_LayerSpec (MultipoleProfileCalculator.h; g_HG unused by the multipole code)
struct MpcLayer {
    float mua, musp, ior, thickness;
};
struct MpcOutput {  // MPC_Output before resampling: the unique-d^2 samples
    std::vector<float> dsq, refl, trans;
    float total_reflectance = 0.f, total_transmittance = 0.f;
};
void mpc_compute(const MpcLayer *layers, int n, float step, int desired_length, bool lerp_on_thin_slab,
                 MpcOutput &out);
void mpc_resample_distribution(const MpcOutput &in, int n, const float *points, float *refl, float *trans);
// MultipoleReferenceTask (mcprofile.cpp:381-425): ring-centre profile of the layers' multipole model
void mc_reference_profile(const MpcLayer *layers, int n, double extent, int nsegments, bool lerp_on_thin_slab,
                          double *refl, double *trans, double *total_r, double *total_t, int desired_length = 1024);
// The same for nslabs two-layer stacks on the current HIP device (profile_gpu.hip): layers [nslabs][2],
// extent [nslabs], outputs [nslabs][nsegments] (nullable) and [nslabs]. Slabs go through the transform
// grids in batches of at most max_batch (0: as many as 8 GB of grids hold; one slab's four grids take
// 1 GiB at desired_length 1024); a slab's result does not depend on the split. Synchronous on stream.
void mc_reference_batch_gpu(const MpcLayer *layers, int nslabs, const double *extent, int nsegments,
                            int desired_length, bool lerp_on_thin_slab, int max_batch, double *refl, double *trans,
                            double *total_r, double *total_t, hipStream_t stream);

// ComputeMonteCarloProfile's ring -> table conversion (multipole.cpp:328-355) for one band
void profile_from_rings(const double *refl, int nseg, double extent, int target, std::vector<float> &table,
                        float &rcp, float &spacing);
// usemontecarlo (multipole.cpp:298-368): per band, a GPU random walk of `photons` photons over
// 4096 rings within 12 mean free paths, resampled to 65536 entries uniform in d^2 (mc_profile.hip)
void build_profile_mc(const LayerParams &lp, uint64_t photons, uint64_t seed, ProfileTables &out);

}  // namespace mpss
