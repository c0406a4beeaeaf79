"""Renderer "multipoleprofilefit" (src/renderers/profilefit.cpp): sum-of-Gaussians coefficients of the
layered-skin multipole profile over a grid of f_mel x f_eu x f_blood x f_ohg, for a real-time renderer.

run() fits a grid on a GPU context (mpss_profile_fit) or on the host (mpss_host_profile_fit); write_table()
writes the reference's tab-separated text table (DoProfileFit, profilefit.cpp:333-378).
"""
import numpy as np

import mpss

PARAMS = ("f_mel", "f_eu", "f_blood", "f_ohg")


def wavelength(band):
    """SampledSpectrum::WaveLength: the centre of band `band` of 30 over 400..700 nm."""
    return 400.0 + (band + 0.5) * (700.0 - 400.0) / mpss.NB


def run(ranges, layers=None, desired_length=256, id_range=(0, -1), ctx=None, max_profiles_per_batch=0, timing=False):
    """ranges: dict of the four parameter lists; layers: [(thickness_nm, ior)] * 2 or None for the fork's
    default skin layers. ctx: an mpss.Context (the GPU path), or None for the host restatement.
    Returns (result dict as mpss.host_profile_fit, the first id of the result)."""
    kw = {}
    if layers is not None:
        kw = dict(layer_thickness_nm=[layers[0][0], layers[1][0]], layer_ior=[layers[0][1], layers[1][1]])
    fit = mpss.profile_fit_spec(desired_length=desired_length, id_range=id_range,
                          max_profiles_per_batch=max_profiles_per_batch, **{k: ranges[k] for k in PARAMS}, **kw)
    res = ctx.profile_fit(fit, timing=timing) if ctx is not None else mpss.host_profile_fit(fit)
    return res, max(0, int(id_range[0]))


def _g(v):
    return "%g" % v  # an ostream's default float format: 6 significant digits


def write_table(out, ranges, res, id_min=0):
    """DoProfileFit's table (profilefit.cpp:341-376) to the text stream `out`. The header block (the ranges and
    the sigma list) is written only when the id range starts at 0, so that the tables of several id ranges
    concatenate into one."""
    rng = [np.sort(np.asarray(ranges[k], np.float32)) for k in PARAMS]
    sig = res["sigmas"]
    if id_min == 0:
        out.write("Param\tNum Samples\tSample Points\n")
        for name, r in zip(PARAMS, rng):
            out.write(name + "\t" + "\t".join([str(len(r))] + [_g(v) for v in r]) + "\n")
        out.write("ID\tf_mel\tf_eu\tf_blood\tf_ohg\tRGB" + "".join("\t" + _g(s) for s in sig) + "\tError\n")
    for i in range(len(res["coeffs"])):
        ident = id_min + i
        rem, vps = ident, [0.0] * 4
        for k in (3, 2, 1, 0):  # ParamsFromId: f_ohg innermost
            vps[k] = rng[k][rem % len(rng[k])]
            rem //= len(rng[k])
        head = str(ident) + "\t" + "\t".join(_g(v) for v in vps) + "\t"
        for sc in range(mpss.NB):
            out.write(head + _g(wavelength(sc)) + "".join("\t" + _g(v) for v in res["coeffs"][i, sc]) + "\t" +
                      _g(res["error"][i, sc]) + "\n")
        for k, ch in enumerate("RGB"):
            out.write(head + ch + "".join("\t" + _g(v) for v in res["rgb_coeffs"][i, k]) + "\n")
