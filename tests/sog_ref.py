"""The yardstick of the sum-of-Gaussians tests: GF_FitSumGaussians + DoGaussianFit restated in float64 numpy
from the algorithm (gaussianfit.cpp:42-154, profilefit.cpp:203-255), in the reference's arithmetic order.

What makes it comparable bit for bit with a C++ restatement:
  * exp goes through math.exp, i.e. the C library's exp (numpy's own vectorised exp may round differently);
  * every running sum is np.cumsum(...)[-1], which adds left to right like the reference's `+=` loop
    (np.sum pairs its terms); `reverse` adds right to left instead -- the same reference arithmetic in the
    other order, used to measure how far a reordering alone moves the coefficients;
  * products are written with the reference's association, in IEEE doubles without contraction;
  * the solve is LinearSolve with its quirk: the pivot row is looked up in the ORIGINAL matrix. quirk=False
    looks it up in the partly eliminated matrix (a textbook partial pivot) to show the difference.
"""
import ctypes as C
import math

import numpy as np

PI_F = float(np.float32(3.141592654))  # numutil.h:45, a float
NEG, TERMS = 3, 6                      # sigmaNegExtent, nTargetSigmas


def linear_solve(a, b, quirk=True):
    with np.errstate(all="ignore"):  # a zero pivot divides to inf / nan as in C, it does not raise
        return _linear_solve(a, b, quirk)


def _linear_solve(a, b, quirk):
    n = len(b)
    a = [[np.float64(v) for v in row] for row in np.asarray(a, np.float64)]
    aa = [row[:] for row in a]
    bb = [np.float64(v) for v in b]
    for row in range(n - 1):
        src = a if quirk else aa
        pivot, max_abs = row, abs(src[row][row])
        for row2 in range(row + 1, n):
            if abs(src[row2][row]) > max_abs:
                max_abs, pivot = abs(src[row2][row]), row2
        if max_abs > 0:
            if pivot != row:
                for c in range(row, n):
                    aa[row][c], aa[pivot][c] = aa[pivot][c], aa[row][c]
                bb[row], bb[pivot] = bb[pivot], bb[row]
            div = aa[row][row]
            aa[row][row] = np.float64(1.0)
            for c in range(row + 1, n):
                aa[row][c] /= div
            bb[row] /= div
            for row2 in range(row + 1, n):
                for c2 in range(row + 1, n):
                    aa[row2][c2] -= aa[row2][row] * aa[row][c2]
                bb[row2] -= aa[row2][row] * bb[row]
    res = [np.float64(0.0)] * n
    for row in range(n - 1, -1, -1):
        rem = bb[row]
        for c in range(n - 1, row, -1):
            rem -= aa[row][c] * res[c]
        res[row] = rem / aa[row][row]
    return np.array(res, np.float64)


def gaussians(dist_sq, sigmas):
    """r (float64 of sqrtf(d^2)) and G[i, s] = exp(-(r r) / (2 sigma sigma)) for every sigma of the list."""
    r = np.sqrt(np.asarray(dist_sq, np.float32)).astype(np.float64)
    rr = r * r
    G = np.empty((len(r), len(sigmas)), np.float64)
    for s, sg in enumerate(np.asarray(sigmas, np.float32)):
        den = 2 * float(sg) * float(sg)
        G[:, s] = [math.exp(-(v / den)) for v in rr.tolist()]
    return r, G


def _seq(v, reverse):
    return float(np.cumsum(v[::-1] if reverse else v)[-1])


def fit_window(r, G6, y, sig6, reverse=False, quirk=True):
    """One window: r, G6 (length, 6) from gaussians(), y float32 data, sig6 float32. Returns (normalised
    coefficients float32[6], overallError float32, X float64 6x6, B float64[6])."""
    y = np.asarray(y, np.float32).astype(np.float64)
    X = np.empty((6, 6), np.float64)
    Y = np.empty(6, np.float64)
    for j in range(6):
        Y[j] = _seq(G6[:, j] * y, reverse)
        for k in range(6):
            X[j, k] = _seq(G6[:, j] * G6[:, k], reverse)
    B = linear_solve(X, Y, quirk)
    fitted = np.zeros(len(r), np.float64)
    for j in range(6):
        fitted = fitted + B[j] * G6[:, j]
    dr = r - np.concatenate([[0.0], r[:-1]])
    error = _seq(r * (fitted - y) * (fitted - y) * dr, False)
    total = _seq(r * y * y * dr, False)
    with np.errstate(all="ignore"):
        err = np.float32(math.sqrt(error / total)) if total > 0 and error / total >= 0 else np.float32(np.nan)
        coeff = np.array([B[k] * 2 * PI_F * float(sig6[k]) * float(sig6[k]) for k in range(6)]).astype(np.float32)
    return coeff, err, X, B


def candidates(sigmas, mfp_min, mfp_max):
    """DoGaussianFit's candidate centres (profilefit.cpp:222-225): float comparisons."""
    sig = np.asarray(sigmas, np.float32)
    lo = np.float32(mfp_min) / np.float32(2)
    hi = np.float32(mfp_max) * np.float32(2)
    out = []
    for c in range(NEG, len(sig) - (TERMS - NEG - 1)):
        if sig[c] < lo:
            continue
        if sig[c] > hi:
            break
        out.append(c)
    return out


def fit_profile(dist_sq, y, sigmas, mfp_min, mfp_max, reverse=False, quirk=True):
    """DoGaussianFit of one profile: dict of cand (centres), cand_coeffs {c: float32[6]}, cand_error {c},
    gram {c: X}, B {c: the unnormalised float64 solution}, centre, error, coeffs (the n_sigmas-wide row)."""
    sig = np.asarray(sigmas, np.float32)
    r, G = gaussians(dist_sq, sig)
    res = dict(cand=candidates(sig, mfp_min, mfp_max), cand_coeffs={}, cand_error={}, gram={}, B={})
    best, best_err = -1, np.float32(np.inf)
    for c in res["cand"]:
        w = slice(c - NEG, c - NEG + TERMS)
        co, er, X, B = fit_window(r, G[:, w], y, sig[w], reverse, quirk)
        res["cand_coeffs"][c], res["cand_error"][c], res["gram"][c], res["B"][c] = co, er, X, B
        if er < best_err:  # strict <, ascending centres: the first of equal errors wins
            best, best_err = c, er
    row = np.zeros(len(sig), np.float32)
    if best >= 0:
        row[best - NEG:best - NEG + TERMS] = res["cand_coeffs"][best]
    res.update(centre=best, error=best_err if best >= 0 else np.float32(np.nan), coeffs=row)
    return res


def sigma_list(mfp_min, mfp_max):
    out = []
    s = np.float32(mfp_min) / np.float32(8)
    top = np.float32(mfp_max) * np.float32(8)
    while s <= top:
        out.append(s)
        s = np.float32(s * np.float32(2))
    return np.array(out, np.float32)


def oracle_fit_profile(oracle, layers, desired_length):
    """One channel as GaussianFitTask::Run builds it, by the oracle (kissfft): layers = [(mua, musp, ior,
    thickness)] * 2 in mm; step 12 mean-mfp / desired_length, lerp on thin slabs, resampled to the sample
    count itself. Returns (d^2, R) float32."""
    mfp = np.float32(0)
    for mua, musp, _, _ in layers:
        mfp = np.float32(mfp + np.float32(1) / (np.float32(mua) + np.float32(musp)))
    mfp = np.float32(mfp / np.float32(2))
    step = np.float32(np.float32(12) * mfp / np.float32(desired_length))
    d, R, _, _, _ = oracle.mpc_profile([(ior, th, mua, musp) for mua, musp, ior, th in layers], float(step),
                                       desired_length, lerp=True, resample=False)
    n = len(d)
    f = oracle.lib().o_mpc_resample_uniform
    f.restype = None
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    out = np.zeros(n, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    R = np.ascontiguousarray(R, np.float32)
    f(n, d.ctypes.data, R.ctypes.data, n, out.ctypes.data)
    i = np.arange(n, dtype=np.float32)
    dsq = (i * d[-1] / np.float32(n - 1)).astype(np.float32)
    return dsq, out


# ---- the shared inputs of the fit tests: a 2 x 1 x 2 x 2 grid (8 ids, 240 profiles) on the fork's default layers
GRID = dict(f_mel=[0.01, 0.1], f_eu=[0.5], f_blood=[0.002, 0.05], f_ohg=[0.3, 0.9])
_CACHE = {}


def grid_case(mpss, desired_length):
    """Host profiles and host fit of GRID at desired_length, computed once per session: dict of fit (the
    mpss.profile_fit_spec tuple), host (mpss.host_profile_fit with profiles), dist_sq / data (240, L), mfp_min /
    mfp_max (240,), sog (mpss.host_sog_fit of those arrays, with the Gram matrices)."""
    if desired_length not in _CACHE:
        fit = mpss.profile_fit_spec(desired_length=desired_length, **GRID)
        host = mpss.host_profile_fit(fit, profiles=True)
        L = host["dist_sq"].shape[2]
        lo, hi = mpss.profilefit_mfp_bounds(fit, range(8))
        d, y = host["dist_sq"].reshape(-1, L), host["data"].reshape(-1, L)
        sog = mpss.host_sog_fit(d, y, host["sigmas"], lo.ravel(), hi.ravel(), gram=True)
        _CACHE[desired_length] = dict(fit=fit, host=host, dist_sq=d, data=y, mfp_min=lo.ravel(), mfp_max=hi.ravel(),
                                      sog=sog)
    return _CACHE[desired_length]


def ambiguous(cand_error):
    """DoGaussianFit's choice is a near-tie: best and second-best overallError within 1e-5 relative."""
    out = np.zeros(len(cand_error), bool)
    for p, row in enumerate(cand_error):
        e = np.sort(row[np.isfinite(row)].astype(np.float64))
        out[p] = len(e) > 1 and (e[1] - e[0]) < 1e-5 * e[1]
    return out


def fitted_curve(sigmas, coeff_row, r):
    """The fitted sum of Gaussians at distances r, float64, from a row of normalised coefficients."""
    out = np.zeros(len(r), np.float64)
    for s, k in zip(np.asarray(sigmas, np.float64), np.asarray(coeff_row, np.float64)):
        if k != 0.0:
            out += k / (2 * math.pi * s * s) * np.exp(-(r * r) / (2 * s * s))
    return out


def weighted_norm(r, v):
    """sqrt(sum r v^2 dr), the error term's own weight (gaussianfit.cpp:138-139)."""
    dr = r - np.concatenate([[0.0], r[:-1]])
    return math.sqrt(float(np.sum(r * v * v * dr)))


def term_norms(sigmas, coeff_row, r, y):
    """The summed weighted norms of the terms k_j g_j of a fitted curve, relative to the data's norm: what one
    float rounding of every returned coefficient can move the curve by, in units of 2^-24."""
    tot = 0.0
    for j, k in enumerate(np.asarray(coeff_row, np.float64)):
        if k != 0.0:
            one = np.zeros(len(coeff_row))
            one[j] = k
            tot += weighted_norm(r, fitted_curve(sigmas, one, r))
    return tot / weighted_norm(r, np.asarray(y, np.float64))


def curve_distance(sigmas, r, y, row_a, row_b):
    """The distance of two fitted curves in the error term's weighted norm, relative to the data's norm."""
    return weighted_norm(r, fitted_curve(sigmas, row_a, r) - fitted_curve(sigmas, row_b, r)) / \
        weighted_norm(r, np.asarray(y, np.float64))
