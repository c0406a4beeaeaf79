// profile_fit_driver.h -- Renderer "multipoleprofilefit" end to end: DoProfileFit's plan over a mpss_profilefit
// grid, then every id's 30 profiles and their sum-of-Gaussians fits, on the context's device or on the host.
// Outputs as mpss_profile_fit / mpss_host_profile_fit (include/mpss.h) document them.
#pragma once
#include "../../include/mpss.h"
#include "material.h"

namespace mpss {

class Context;

// combination `id` of the grid: its four parameters and (lp non-null) its layers; `who` prefixes the message
void profile_fit_id(const char *who, const mpss_profilefit &f, uint32_t id, float params[4], LayerParams *lp);
void profile_fit_gpu(Context &ctx, const mpss_profilefit &f, uint32_t *n_sigmas, uint32_t *n_ids, float *sigmas,
                     float *coeffs, float *error, float *rgb, int32_t *centre, double *stage_ms, hipStream_t stream);
void profile_fit_host(const mpss_profilefit &f, uint32_t *n_sigmas, uint32_t *n_ids, float *sigmas, float *coeffs,
                      float *error, float *rgb, int32_t *centre, uint32_t *length, float *pd, float *py);

}  // namespace mpss
