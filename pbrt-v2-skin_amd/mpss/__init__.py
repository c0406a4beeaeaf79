"""mpss -- Python host binding of libmpss (the MI355X-native multipole subsurface path).

Thin ctypes layer over the C ABI in include/mpss.h.  Device buffers are passed as raw
HIP pointers (torch CUDA tensors' ``data_ptr()``); torch is plumbing here, not the product.
The HIP library is mandatory: importing this module raises if libmpss.so is missing, and
there is no CPU fallback anywhere in the product path.
"""
import ctypes as C
import os

import numpy as np

NB = 30
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPSS_LIB") or os.path.join(_HERE, "libmpss.so")  # MPSS_LIB: a variant build (tools/)

if not os.path.exists(LIB_PATH):
    raise ImportError("libmpss.so not built (%s): run __graft_entry__.build() or make -C pbrt-v2-skin_amd/csrc"
                      % LIB_PATH)

# torch-ROCm ships its own libamdhip64/libhsa-runtime64 (same SONAME, different NEEDED spelling).
# Loading libmpss first would pull /opt/rocm's runtime in beside torch's and leave two HSA
# runtimes fighting over /dev/kfd; importing torch first makes libmpss bind to torch's copy.
try:
    import torch  # noqa: F401
except ImportError:  # pure C/ctypes use without torch: /opt/rocm's runtime is used
    torch = None

_lib = C.CDLL(LIB_PATH)

f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
vp = C.c_void_p
u32 = C.c_uint32
u32p = C.POINTER(C.c_uint32)


class Config(C.Structure):
    """mpss_config (CreateMultipoleSubsurfaceIntegrator params, multipolesubsurface.cpp:393-401)."""
    _fields_ = [("device", C.c_int), ("max_depth", C.c_int), ("max_error", C.c_float),
                ("min_sample_distance", C.c_float), ("mix", C.c_float), ("show_irradiance_points", C.c_int),
                ("incenter", C.c_int), ("quick_render", C.c_int), ("exact_mo", C.c_int),
                ("kernel_timing", C.c_int), ("count_traversal", C.c_int), ("profile_on_host", C.c_int),
                ("max_batch_samples", C.c_int64), ("use_poisson_point_finder", C.c_int), ("sampler", C.c_int),
                ("replay_cores", C.c_int), ("octree_on_host", C.c_int), ("mo_band_dealing", C.c_int),
                ("mo_work_stealing", C.c_int), ("mo_near_field", C.c_int), ("tessellate_on_host", C.c_int),
                ("mo_common_grid", C.c_int)]

SAMPLER_HASH, SAMPLER_REFERENCE = 0, 1


class RenderStats(C.Structure):
    """mpss_render_stats."""
    _fields_ = [("ms_irradiance", C.c_double), ("ms_camera", C.c_double), ("ms_shade", C.c_double),
                ("ms_film", C.c_double), ("n_irradiance", C.c_int64), ("n_camera", C.c_int64),
                ("n_shade", C.c_int64), ("n_film", C.c_int64), ("samples", C.c_int64), ("sss_samples", C.c_int64),
                ("mo_nodes", C.c_int64), ("mo_points", C.c_int64), ("group_nodes", C.c_int64 * 8),
                ("group_points", C.c_int64 * 8), ("group_bands", (C.c_int32 * 4) * 8), ("ms_direct", C.c_double),
                ("n_direct", C.c_int64), ("mo_wave_node_iters", C.c_int64), ("mo_wave_point_iters", C.c_int64),
                ("mo_lookups", C.c_int64), ("mo_lookups_near", C.c_int64 * 3), ("mo_row_lane_records", C.c_int64),
                ("mo_lds_lane_records", C.c_int64), ("mo_table_lane_records", C.c_int64), ("ms_tex", C.c_double),
                ("n_tex", C.c_int64), ("ms_replay", C.c_double), ("n_replay", C.c_int64),
                ("group_path_records", (C.c_int64 * 3) * 8), ("group_path_sectors", (C.c_int64 * 2) * 8),
                ("group_path_lines", (C.c_int64 * 2) * 8), ("group_path_fetches", (C.c_int64 * 2) * 8)]


class LayeredSkin(C.Structure):
    """mpss_layeredskin (CreateLayeredSkinMaterial params, layeredskin.cpp:234-257)."""
    _fields_ = [("roughness", C.c_float), ("nmperunit", C.c_float), ("f_mel", C.c_float), ("f_eu", C.c_float),
                ("f_blood", C.c_float), ("f_ohg", C.c_float), ("ga_epi", C.c_float), ("ga_derm", C.c_float),
                ("b_derm", C.c_float), ("layer_thickness_nm", C.c_float * 2), ("layer_ior", C.c_float * 2),
                ("albedo", C.c_float * NB), ("Kr", C.c_float * NB), ("Kt", C.c_float * NB),
                ("desired_length", C.c_int), ("lerp_on_thin_slab", C.c_int),
                ("double_ref_sslf", C.c_int), ("use_monte_carlo", C.c_int), ("photons", C.c_uint64),
                ("rgb_profile", C.c_int), ("gen_profile", C.c_int), ("show_irradiance_points", C.c_int),
                ("irradiance_point_size", C.c_float)]


class Imagemap(C.Structure):
    """mpss_imagemap (Texture "imagemap" params, textures/imagemap.cpp:110-180)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("texels", vp), ("is_float", C.c_int),
                ("shift", C.c_float), ("scale", C.c_float), ("gamma", C.c_float), ("wrap", C.c_int),
                ("trilinear", C.c_int), ("max_anisotropy", C.c_float), ("uscale", C.c_float), ("vscale", C.c_float),
                ("udelta", C.c_float), ("vdelta", C.c_float)]


class ProfileFit(C.Structure):
    """mpss_profilefit (Renderer "multipoleprofilefit" params, profilefit.cpp:524-558)."""
    _fields_ = [("f_mel", C.POINTER(C.c_float)), ("f_eu", C.POINTER(C.c_float)), ("f_blood", C.POINTER(C.c_float)),
                ("f_ohg", C.POINTER(C.c_float)), ("n_f_mel", C.c_uint32), ("n_f_eu", C.c_uint32),
                ("n_f_blood", C.c_uint32), ("n_f_ohg", C.c_uint32), ("layer_thickness_nm", C.c_float * 2),
                ("layer_ior", C.c_float * 2), ("desired_length", C.c_int), ("id_min", C.c_int), ("id_max", C.c_int),
                ("max_profiles_per_batch", C.c_int)]


def _sig(name, res, args):
    f = getattr(_lib, name)
    f.restype = res
    f.argtypes = args
    return f


_sig("mpss_abi_version", C.c_int, [])
_sig("mpss_last_error", C.c_char_p, [])
_sig("mpss_config_defaults", None, [C.POINTER(Config)])
_sig("mpss_create", C.c_int, [C.POINTER(Config), C.POINTER(vp)])
_sig("mpss_destroy", None, [vp])
_sig("mpss_layeredskin_defaults", None, [C.POINTER(LayeredSkin)])
_sig("mpss_add_layeredskin", C.c_int, [vp, C.POINTER(LayeredSkin), u32p])
_sig("mpss_update_layeredskin", C.c_int, [vp, u32, C.POINTER(LayeredSkin)])
_sig("mpss_build_counts", C.c_int, [vp, C.POINTER(C.c_uint64)])
_sig("mpss_get_common_grid", C.c_int, [vp, u32, C.c_int, vp, u32p] + [vp] * 11 + [C.POINTER(C.c_int)])
_sig("mpss_set_grid_builder", C.c_int, [vp, C.c_int])
_sig("mpss_set_pixel_filter", C.c_int, [vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float])
_sig("mpss_set_material_tables", C.c_int, [vp, f32p, u32, f32p, f32p, u32, vp, C.c_int, u32p])
_sig("mpss_add_dipole_material", C.c_int, [vp, f32p, f32p, C.c_float, u32p])
_sig("mpss_host_dipole_rd", C.c_int, [f32p, f32p, C.c_float, u32, vp, vp, vp])
_sig("mpss_get_material_tables", C.c_int, [vp, u32, vp, u32p, vp, vp, u32p, vp])
_sig("mpss_get_gather_info", C.c_int, [vp, u32, C.POINTER(C.c_int), vp, vp])
_sig("mpss_set_irradiance_points", C.c_int, [vp, u32, f32p, f32p, f32p, f32p])
_sig("mpss_octree_info", C.c_int, [vp, u32p, u32p, u32p])
_sig("mpss_octree_export", C.c_int, [vp, vp, vp, vp, vp, vp])
_sig("mpss_mo_batch", C.c_int, [vp, u32, u32, vp, vp, vp, vp])
_sig("mpss_mo_batch_paths", C.c_int, [vp, u32, u32, vp, vp, vp])
_sig("mpss_add_mesh", C.c_int, [vp, u32, f32p, vp, vp, vp, u32, C.POINTER(C.c_int32), f32p, f32p, C.c_int, u32])
_sig("mpss_add_sphere_light", C.c_int, [vp, f32p, C.c_float, f32p, C.c_int])
_sig("mpss_add_infinite_light", C.c_int, [vp, f32p, C.c_int, f32p, f32p])
_sig("mpss_add_infinite_light_map", C.c_int, [vp, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, f32p])
_sig("mpss_set_camera", C.c_int, [vp, f32p, f32p, C.c_int, C.c_int])
_sig("mpss_set_surface_points", C.c_int, [vp, u32, vp])
_sig("mpss_get_surface_points", C.c_int, [vp, vp, u32p])
_sig("mpss_get_irradiance", C.c_int, [vp, vp, u32p])
_sig("mpss_replay_samples", C.c_int, [vp, C.c_int, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int)])
_sig("mpss_load_pointsfile", C.c_int, [vp, C.c_char_p])
_sig("mpss_save_pointsfile", C.c_int, [vp, C.c_char_p])
_sig("mpss_preprocess", C.c_int, [vp, u32])
_sig("mpss_get_render_stats", C.c_int, [vp, C.POINTER(RenderStats)])
_sig("mpss_reset_render_stats", C.c_int, [vp])
_sig("mpss_set_instrumentation", C.c_int, [vp, C.c_int, C.c_int])
_sig("mpss_render_tile", C.c_int, [vp, C.c_int, u32, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp])
_sig("mpss_render_tiles", C.c_int, [vp, C.c_int, u32, C.c_int, C.POINTER(C.c_int32), C.POINTER(vp), vp])
_sig("mpss_render_tile_spectral", C.c_int, [vp, C.c_int, u32, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp])
_sig("mpss_render_tiles_spectral", C.c_int, [vp, C.c_int, u32, C.c_int, C.POINTER(C.c_int32), C.POINTER(vp),
                                             C.POINTER(vp), vp])
_sig("mpss_tile_costs", C.c_int, [vp, C.c_int, C.POINTER(C.c_int32), vp, vp])
_sig("mpss_host_from_rgb", C.c_int, [f32p, C.c_int, f32p])
_sig("mpss_host_spectrum_to_xyz", C.c_int, [f32p, u32, f32p])
_sig("mpss_mc_reference", C.c_int, [f32p, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)])
_sig("mpss_mc_profile", C.c_int, [vp, f32p, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint64, vp, vp,
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), vp])
_sig("mpss_mc_profile_batch", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint64, vp, vp,
                                        vp, vp, C.POINTER(C.c_uint64), vp])
_sig("mpss_mc_reference_batch", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                          vp, vp, vp, vp, vp])
_sig("mpss_host_tessellate", C.c_int, [u32, f32p, vp, vp, vp, u32, C.POINTER(C.c_int32), f32p, f32p, C.c_int, u32,
                                       C.c_float, C.c_int, vp, u32p])
_sig("mpss_imagemap_defaults", None, [C.POINTER(Imagemap)])
_sig("mpss_add_imagemap", C.c_int, [vp, C.POINTER(Imagemap), u32p])
_sig("mpss_set_material_textures", C.c_int, [vp, u32, C.c_int32, C.c_int32])
_sig("mpss_set_material_spec_textures", C.c_int, [vp, u32, C.c_int32, C.c_int32])
_sig("mpss_host_tessellate_bumped", C.c_int, [u32, f32p, vp, vp, vp, u32, C.POINTER(C.c_int32), f32p, f32p, C.c_int,
                                              u32, C.c_float, C.c_int, vp, vp, u32p])
_sig("mpss_host_imagemap_lookup", C.c_int, [C.POINTER(Imagemap), u32, f32p, f32p])
_sig("mpss_host_skin_layers", C.c_int, [C.POINTER(LayeredSkin), f32p, f32p, f32p, f32p])
_sig("mpss_host_build_profile", C.c_int, [f32p, f32p, f32p, f32p, C.c_int, C.c_int, vp, u32p, vp, vp])
_sig("mpss_host_rho_table", C.c_int, [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, f32p, C.POINTER(C.c_float)])
_sig("mpss_host_common_grid", C.c_int, [f32p, u32, f32p, C.c_int, C.c_int, vp, u32p] + [vp] * 11 + [C.POINTER(C.c_int)])
_sig("mpss_profilefit_defaults", None, [C.POINTER(ProfileFit)])
_sig("mpss_profilefit_params", C.c_int, [C.POINTER(ProfileFit), u32, f32p])
_sig("mpss_profilefit_layers", C.c_int, [C.POINTER(ProfileFit), u32, f32p, f32p, f32p, f32p])
_sig("mpss_profile_fit", C.c_int, [vp, C.POINTER(ProfileFit), u32p, u32p] + [vp] * 6 + [vp])
_sig("mpss_host_profile_fit", C.c_int, [C.POINTER(ProfileFit), u32p, u32p] + [vp] * 5 + [u32p, vp, vp])
_sig("mpss_sog_fit", C.c_int, [vp, u32, u32, f32p, f32p, u32, f32p, f32p, f32p] + [vp] * 5 + [vp])
_sig("mpss_host_sog_fit", C.c_int, [u32, u32, f32p, f32p, u32, f32p, f32p, f32p] + [vp] * 6)
_sig("mpss_host_sog_solve", C.c_int, [vp, vp, C.c_int, vp])
_sig("mpss_host_octree_export", C.c_int, [u32, f32p, f32p, f32p, f32p, u32p] + [vp] * 8)


class MpssError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise MpssError("libmpss error %d: %s" % (rc, _lib.mpss_last_error().decode()))


def lib():
    return _lib


def exported_symbols():
    """Names declared in include/mpss.h (checked by tests/test_abi.py)."""
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "mpss.h")
    txt = open(hdr).read()
    return sorted(set(re.findall(r"\b(mpss_[a-z0-9_]+)\s*\(", txt)))


def default_config(**kw):
    c = Config()
    _lib.mpss_config_defaults(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def default_skin(**kw):
    m = LayeredSkin()
    _lib.mpss_layeredskin_defaults(C.byref(m))
    for k, v in kw.items():
        if k in ("layer_thickness_nm", "layer_ior"):
            setattr(m, k, (C.c_float * 2)(*v))
        elif k in ("albedo", "Kr", "Kt"):
            setattr(m, k, (C.c_float * NB)(*v))
        else:
            setattr(m, k, v)
    return m


_WRAP = {"repeat": 0, "black": 1, "clamp": 2}


def imagemap(texels=None, is_float=False, shift=0.0, scale=1.0, gamma=1.0, wrap="repeat", trilinear=False,
             maxanisotropy=8.0, uscale=1.0, vscale=1.0, udelta=0.0, vdelta=0.0):
    """An mpss_imagemap for an (H, W, 3) texel array (ReadImage's RGB, mpss.imageio), or for an
    image that could not be read (texels None: the reference's one-valued map). Returns (struct,
    the array it points at -- keep it alive while the struct is used)."""
    t = Imagemap()
    _lib.mpss_imagemap_defaults(C.byref(t))
    arr = None
    if texels is not None:
        arr = np.ascontiguousarray(texels, np.float32)
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("texels must be (height, width, 3)")
        t.height, t.width = arr.shape[:2]
        t.texels = arr.ctypes.data
    t.is_float = int(bool(is_float))
    t.shift, t.scale, t.gamma = float(shift), float(scale), float(gamma)
    if wrap not in _WRAP:
        raise ValueError("wrap mode %r" % wrap)
    t.wrap = _WRAP[wrap]
    t.trilinear = int(bool(trilinear))
    t.max_anisotropy = float(maxanisotropy)
    t.uscale, t.vscale, t.udelta, t.vdelta = float(uscale), float(vscale), float(udelta), float(vdelta)
    return t, arr


def host_imagemap_lookup(tex, uvd):
    """ImageTexture::Evaluate of the product's host code: tex = imagemap(...) kwargs dict;
    uvd (n, 6) = u, v, dudx, dvdx, dudy, dvdy -> (n, 3) MIPMap values."""
    t, keep = imagemap(**tex)
    uvd = np.ascontiguousarray(uvd, np.float32).reshape(-1, 6)
    out = np.zeros((len(uvd), 3), np.float32)
    check(_lib.mpss_host_imagemap_lookup(C.byref(t), len(uvd), uvd, out))
    del keep
    return out


# SurfacePoint record, the "pointsfile" format (renderers/surfacepoints.h:45-55), 44 B.
SURFACE_POINT = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("material", "<u4"),
                          ("area", "<f4"), ("ray_eps", "<f4")])
assert SURFACE_POINT.itemsize == 44


# ------------------------------------------------------------------ host utilities
def host_from_rgb(rgb, illuminant=False):
    out = np.zeros(NB, np.float32)
    check(_lib.mpss_host_from_rgb(np.ascontiguousarray(rgb, np.float32), int(illuminant), out))
    return out


SPECTRAL_ROW = 32  # MPSS_SPECTRAL_ROW: 30 band sums, the weight sum, 0


def host_spectrum_to_xyz(spec):
    """Spectrum::ToXYZ in band order (mpss_host_spectrum_to_xyz): spec (..., 30) -> (..., 3) float32."""
    spec = np.ascontiguousarray(spec, np.float32)
    if spec.shape[-1] != NB:
        raise ValueError("spectra must have %d bands" % NB)
    out = np.zeros(spec.shape[:-1] + (3,), np.float32)
    check(_lib.mpss_host_spectrum_to_xyz(spec.reshape(-1), spec.size // NB, out.reshape(-1)))
    return out


def host_tessellate(P, idx, o2w, w2o, min_dist, N=None, S=None, uv=None, flip=False, material=0, incenter=False,
                    bump=None):
    """TessellateSurfacePoints of one mesh by the product's host code; bump: imagemap(...) kwargs
    dict of a float "bumpmap" texture, or None."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    opt = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (N, S, uv)]
    args = [len(P), P] + [None if a is None else a.ctypes.data for a in opt] + \
        [len(idx), idx.ctypes.data_as(C.POINTER(C.c_int32)), np.ascontiguousarray(o2w, np.float32),
         np.ascontiguousarray(w2o, np.float32), int(flip), material, min_dist, int(incenter)]
    bt, keep = imagemap(**bump) if bump is not None else (None, None)
    args.append(C.byref(bt) if bt is not None else None)
    n = C.c_uint32(0)
    check(_lib.mpss_host_tessellate_bumped(*args, None, C.byref(n)))
    out = np.zeros(n.value, SURFACE_POINT)
    check(_lib.mpss_host_tessellate_bumped(*args, out.ctypes.data, C.byref(n)))
    del keep
    return out


def host_skin_layers(skin):
    mua = np.zeros((2, NB), np.float32)
    musp = np.zeros((2, NB), np.float32)
    th = np.zeros(2, np.float32)
    eta = np.zeros(2, np.float32)
    check(_lib.mpss_host_skin_layers(C.byref(skin), mua, musp, th, eta))
    return mua, musp, th, eta


def host_build_profile(mua, musp, thickness, eta, desired_length=512, lerp=True):
    args = [np.ascontiguousarray(x, np.float32) for x in (mua, musp, thickness, eta)]
    n = C.c_uint32()
    check(_lib.mpss_host_build_profile(*args, desired_length, int(lerp), None, C.byref(n), None, None))
    # the length query above ran the whole build; run once more into buffers
    tab = np.zeros((NB, n.value), np.float32)
    rcp = np.zeros(NB, np.float32)
    tot = np.zeros(NB, np.float32)
    check(_lib.mpss_host_build_profile(*args, desired_length, int(lerp), tab.ctypes.data, C.byref(n),
                                       rcp.ctypes.data, tot.ctypes.data))
    return tab, rcp, tot


def mc_reference(layers, mfp_range=16.0, nsegments=1024, lerp=True):
    """MultipoleReferenceTask (mcprofile.cpp:356-425): the multipole model of `layers`
    [(mua, musp, ior, thickness), ...] at the MC profile's ring centres; host code."""
    lay = np.ascontiguousarray(layers, np.float32).reshape(-1, 4)
    r = np.zeros(nsegments, np.float64)
    t = np.zeros(nsegments, np.float64)
    tr, tt = C.c_double(), C.c_double()
    check(_lib.mpss_mc_reference(lay, len(lay), mfp_range, nsegments, int(lerp), r.ctypes.data, t.ctypes.data,
                                 C.byref(tr), C.byref(tt)))
    return dict(reflectance=r, transmittance=t, total_r=tr.value, total_t=tt.value)


def mc_extent(layers, mfp_range=16.0):
    """The MC profile's tally radius per slab (Render, mcprofile.cpp:457-463): mfp_range x the mean over
    layers of 1 / (mua + musp), the sum in float, the rest in double. layers [S, n, 4] -> [S]."""
    lay = np.asarray(layers, np.float32)
    mfp = (1.0 / (lay[..., 0] + lay[..., 1]).astype(np.float64)).sum(axis=-1) / lay.shape[-2]
    return float(np.float32(mfp_range)) * mfp


def host_dipole_rd(sigma_a, sigmap_s, eta, d2):
    """DiffusionReflectance(sigma_a, sigmap_s, eta)(d2) per squared distance (n x 30) and its
    TotalReflectance() (diffusionutil.h:38-83)."""
    d2 = np.ascontiguousarray(np.atleast_1d(d2), np.float32)
    rd = np.zeros((len(d2), NB), np.float32)
    tot = np.zeros(NB, np.float32)
    check(_lib.mpss_host_dipole_rd(np.ascontiguousarray(sigma_a, np.float32), np.ascontiguousarray(sigmap_s, np.float32),
                                   eta, len(d2), d2.ctypes.data, rd.ctypes.data, tot.ctypes.data))
    return rd, tot


def host_rho_table(roughness, eta, n=1025, sqrt_samples=256, double_ref_sslf=False):
    hd = np.zeros(n, np.float32)
    hh = C.c_float()
    check(_lib.mpss_host_rho_table(roughness, eta, int(double_ref_sslf), n, sqrt_samples, hd, C.byref(hh)))
    return hd, hh.value


def host_common_grid(table, rcp, snake=False, rgb=False, near_field=5088):
    """The sharded gather's common grid for a profile (mpss_host_common_grid): dict of rows
    (n_rows, 8), bands (8, 4), rg, u0lim, u1lim, u1start, row0, ubase (8,), rel_err / l1_err (30,),
    ok. rgb: an rgbprofile table (rows 0..2 in every group). near_field: the LDS layout the grid is
    built for (mpss_config.mo_near_field; 5088 is the default)."""
    table = np.ascontiguousarray(table, np.float32)
    rcp = np.ascontiguousarray(rcp, np.float32)
    L = table.shape[1]
    mode = 2 if rgb else int(snake)
    n = C.c_uint32(0)
    nul = [None] * 11
    ok = C.c_int()
    check(_lib.mpss_host_common_grid(table, L, rcp, mode, int(near_field), None, C.byref(n), *nul, C.byref(ok)))
    out = dict(rows=np.zeros((n.value, 8), np.float32), bands=np.zeros((8, 4), np.int32),
               rg=np.zeros(8, np.float32), u0lim=np.zeros(8, np.float32), u1lim=np.zeros(8, np.float32),
               u1start=np.zeros(8, np.float32), row0=np.zeros(8, np.uint32), ubase=np.zeros(8, np.uint32),
               rel_err=np.zeros(NB, np.float32), l1_err=np.zeros(NB, np.float32), ua=np.zeros(8, np.float32),
               hinv=np.zeros(8, np.float32))
    check(_lib.mpss_host_common_grid(table, L, rcp, mode, int(near_field), out["rows"].ctypes.data, C.byref(n),
                                     *[out[k].ctypes.data for k in ("bands", "rg", "u0lim", "u1lim", "u1start", "row0",
                                                                    "ubase", "rel_err", "l1_err", "ua", "hinv")],
                                     C.byref(ok)))
    out["ok"] = bool(ok.value)
    return out


def host_octree_export(p, n, E, area):
    p, n, E, area = [np.ascontiguousarray(x, np.float32) for x in (p, n, E, area)]
    nn = C.c_uint32()
    check(_lib.mpss_host_octree_export(len(p), p, n, E, area, C.byref(nn), *([None] * 8)))
    N = nn.value
    d = dict(p=np.zeros((N, 3), np.float32), area=np.zeros(N, np.float32), Et=np.zeros((N, NB), np.float32),
             depth=np.zeros(N, np.int32), skip=np.zeros(N, np.int32), leaf_first=np.zeros(N, np.int32),
             leaf_count=np.zeros(N, np.int32), order=np.zeros(len(p), np.int32))
    check(_lib.mpss_host_octree_export(len(p), p, n, E, area, C.byref(nn),
                                       *[d[k].ctypes.data for k in ("p", "area", "Et", "depth", "skip",
                                                                    "leaf_first", "leaf_count", "order")]))
    return d


# ------------------------------------------------------------------ sum-of-Gaussians profile fit
def profile_fit_spec(f_mel, f_eu, f_blood, f_ohg, layer_thickness_nm=None, layer_ior=None, desired_length=256,
               id_range=(0, -1), max_profiles_per_batch=0):
    """An mpss_profilefit for the four parameter ranges. Returns (struct, arrays it points at -- keep them
    alive while the struct is used)."""
    f = ProfileFit()
    _lib.mpss_profilefit_defaults(C.byref(f))
    keep = []
    for name, vals in (("f_mel", f_mel), ("f_eu", f_eu), ("f_blood", f_blood), ("f_ohg", f_ohg)):
        a = np.ascontiguousarray(np.atleast_1d(vals), np.float32)
        keep.append(a)
        setattr(f, name, a.ctypes.data_as(C.POINTER(C.c_float)))
        setattr(f, "n_" + name, len(a))
    if layer_thickness_nm is not None:
        f.layer_thickness_nm = (C.c_float * 2)(*layer_thickness_nm)
    if layer_ior is not None:
        f.layer_ior = (C.c_float * 2)(*layer_ior)
    f.desired_length = int(desired_length)
    f.id_min, f.id_max = int(id_range[0]), int(id_range[1])
    f.max_profiles_per_batch = int(max_profiles_per_batch)
    return f, keep


def _profile_fit_call(call):
    """sizes first, then one full run; call(ns, ni, sigmas, coeffs, error, rgb, centre)"""
    ns, ni = C.c_uint32(), C.c_uint32()
    check(call(ns, ni, None, None, None, None, None))
    sig = np.zeros(ns.value, np.float32)
    out = dict(sigmas=sig, coeffs=np.zeros((ni.value, NB, ns.value), np.float32),
               error=np.zeros((ni.value, NB), np.float32), rgb_coeffs=np.zeros((ni.value, 3, ns.value), np.float32),
               centre=np.zeros((ni.value, NB), np.int32))
    if ni.value == 0:
        check(call(ns, ni, sig.ctypes.data, None, None, None, None))
        return out
    check(call(ns, ni, sig.ctypes.data, out["coeffs"].ctypes.data, out["error"].ctypes.data,
               out["rgb_coeffs"].ctypes.data, out["centre"].ctypes.data))
    return out


def profilefit_params(fit, ident):
    """ParamsFromId: (f_mel, f_eu, f_blood, f_ohg) of id `ident`; fit = profile_fit_spec(...)."""
    out = np.zeros(4, np.float32)
    check(_lib.mpss_profilefit_params(C.byref(fit[0]), ident, out))
    return out


def profilefit_layers(fit, ident):
    """The layers of id `ident` in millimetres, as the fit builds them: mua, musp (2, 30), thickness, eta (2,)."""
    mua = np.zeros((2, NB), np.float32)
    musp = np.zeros((2, NB), np.float32)
    th = np.zeros(2, np.float32)
    eta = np.zeros(2, np.float32)
    check(_lib.mpss_profilefit_layers(C.byref(fit[0]), ident, mua, musp, th, eta))
    return mua, musp, th, eta


def profilefit_mfp_bounds(fit, ids):
    """Each channel's own mfp bounds (GaussianFitTask::Run, profilefit.cpp:165-173), float32: two arrays
    (len(ids), 30) -- the candidate filter's mfpMin and mfpMax."""
    lo, hi = [], []
    for i in ids:
        mua, musp, _, _ = profilefit_layers(fit, i)
        mfp = np.float32(1) / (mua + musp)
        lo.append(mfp.min(axis=0))
        hi.append(mfp.max(axis=0))
    return np.array(lo, np.float32), np.array(hi, np.float32)


def host_profile_fit(fit, profiles=False):
    """mpss_host_profile_fit: fit = profile_fit_spec(...). dict of sigmas, coeffs (ids, 30, n_sigmas), error
    (ids, 30), rgb_coeffs (ids, 3, n_sigmas), centre (ids, 30); profiles=True adds dist_sq / data
    (ids, 30, length), the resampled profiles the fit read (the same single run fills them)."""
    f = fit[0]
    L = fit_profile_length(f.desired_length) if profiles else 0
    keep = {}

    def call(ns, ni, s, c, e, r, ce):
        d = y = None
        if profiles and c is not None:
            keep["dist_sq"] = np.zeros((ni.value, NB, L), np.float32)
            keep["data"] = np.zeros((ni.value, NB, L), np.float32)
            d, y = keep["dist_sq"].ctypes.data, keep["data"].ctypes.data
        ln = C.c_uint32()
        rc = _lib.mpss_host_profile_fit(C.byref(f), C.byref(ns), C.byref(ni), s, c, e, r, ce, C.byref(ln), d, y)
        assert rc != 0 or d is None or ln.value == L
        return rc

    out = _profile_fit_call(call)
    out.update(keep)
    return out


def fit_profile_length(desired_length):
    """Samples of a profile at desired_length (the unique i^2 + j^2 <= ext^2, ext = the next power of two - 1;
    MultipoleProfileCalculator.cpp:316-330): 87 at 16, 318 at 32, 1162 at 64, 15978 at 256."""
    ext = 1
    while ext < desired_length:
        ext *= 2
    ext -= 1
    i = np.arange(ext + 1, dtype=np.int64)
    n = (i[:, None] ** 2 + i[None, :] ** 2).ravel()
    return len(np.unique(n[n <= ext * ext]))


def _sog_args(dist_sq, data, sigmas, mfp_min, mfp_max):
    d = np.ascontiguousarray(np.atleast_2d(dist_sq), np.float32)
    y = np.ascontiguousarray(np.atleast_2d(data), np.float32)
    assert d.shape == y.shape
    n, L = d.shape
    sig = np.ascontiguousarray(sigmas, np.float32)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(mfp_min, np.float32), (n,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(mfp_max, np.float32), (n,)))
    ns = len(sig)
    out = dict(coeffs=np.zeros((n, ns), np.float32), error=np.zeros(n, np.float32), centre=np.zeros(n, np.int32),
               cand_error=np.zeros((n, ns), np.float32), cand_coeffs=np.zeros((n, ns, 6), np.float32))
    return (n, L, d, y, ns, sig, lo, hi), out


def host_sog_fit(dist_sq, data, sigmas, mfp_min, mfp_max, gram=False):
    """mpss_host_sog_fit: profiles (n, length) of d^2 and R -> dict of coeffs (n, n_sigmas), error, centre,
    cand_error (n, n_sigmas; NaN: no candidate), cand_coeffs (n, n_sigmas, 6), and with gram=True cand_gram
    (n, n_sigmas, 6, 6)."""
    args, out = _sog_args(dist_sq, data, sigmas, mfp_min, mfp_max)
    g = np.zeros((args[0], args[4], 6, 6), np.float64) if gram else None
    check(_lib.mpss_host_sog_fit(*args, out["coeffs"].ctypes.data, out["error"].ctypes.data,
                                 out["centre"].ctypes.data, out["cand_error"].ctypes.data,
                                 out["cand_coeffs"].ctypes.data, g.ctypes.data if gram else None))
    if gram:
        out["cand_gram"] = g
    return out


def host_sog_solve(a, b, quirk=True):
    """LinearSolve (gaussianfit.cpp:48-96) of the library for a 6 x 6 system."""
    a = np.ascontiguousarray(a, np.float64).reshape(6, 6)
    b = np.ascontiguousarray(b, np.float64).reshape(6)
    x = np.zeros(6, np.float64)
    check(_lib.mpss_host_sog_solve(a.ctypes.data, b.ctypes.data, int(quirk), x.ctypes.data))
    return x


# ------------------------------------------------------------------ device context
# pbrt's PixelFilter names in MPSS_FILTER_* order, and per kind (default width, ((parameter, default), ...))
# as core/api.cpp MakeFilter's Create*Filter read them
PIXEL_FILTERS = ("box", "triangle", "gaussian", "mitchell", "sinc")
_FILTER_DEFAULTS = ((0.5, ()), (2.0, ()), (2.0, (("alpha", 2.0),)), (2.0, (("B", 1.0 / 3.0), ("C", 1.0 / 3.0))),
                    (4.0, (("tau", 3.0),)))


def pixel_filter(kind, xwidth=None, ywidth=None, **params):
    """(kind, xwidth, ywidth, a, b) as mpss_set_pixel_filter takes them, the reference's defaults filled
    in. An unknown kind or a parameter the kind does not have raises ValueError."""
    if isinstance(kind, str):
        if kind not in PIXEL_FILTERS:
            raise ValueError("unknown pixel filter %r" % kind)
        kind = PIXEL_FILTERS.index(kind)
    kind = int(kind)
    if not 0 <= kind < len(PIXEL_FILTERS):
        raise ValueError("unknown pixel filter kind %d" % kind)
    width, names = _FILTER_DEFAULTS[kind]
    extra = set(params) - {n for n, _ in names}
    if extra:
        raise ValueError("pixel filter %r has no parameter %s" % (PIXEL_FILTERS[kind], ", ".join(sorted(extra))))
    ab = [float(params.get(n, d)) for n, d in names] + [0.0, 0.0]
    return (kind, float(width if xwidth is None else xwidth), float(width if ywidth is None else ywidth), ab[0], ab[1])


class Context:
    """One MultipoleSubsurfaceIntegrator instance (multipolesubsurface.h:36-80) on one GPU."""

    def __init__(self, **cfg):
        self.cfg = default_config(**cfg)
        h = vp()
        check(_lib.mpss_create(C.byref(self.cfg), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            _lib.mpss_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def add_layeredskin(self, skin):
        mid = C.c_uint32()
        check(_lib.mpss_add_layeredskin(self.h, C.byref(skin), C.byref(mid)))
        return mid.value

    def update_layeredskin(self, mid, skin):
        """mpss_update_layeredskin: material `mid` rebuilt in place for `skin` (id, texture bindings and
        meshes kept). Run preprocess() again before the next render."""
        check(_lib.mpss_update_layeredskin(self.h, mid, C.byref(skin)))

    def build_counts(self):
        """mpss_build_counts: monotonic counts of scene uploads, point-set builds, material table
        builds and octree builds since the context was created."""
        c = (C.c_uint64 * 4)()
        check(_lib.mpss_build_counts(self.h, c))
        return dict(scene_uploads=int(c[0]), point_builds=int(c[1]), material_builds=int(c[2]),
                    octree_builds=int(c[3]))

    def set_grid_builder(self, on_host=True):
        """mpss_set_grid_builder: the common grids' per-knot scan of later material builds on the host
        (True) or on the GPU (False); the same grids either way."""
        check(_lib.mpss_set_grid_builder(self.h, int(bool(on_host))))

    def set_pixel_filter(self, kind, xwidth=None, ywidth=None, **params):
        """mpss_set_pixel_filter: the film's reconstruction filter of later renders. kind: a name of
        PIXEL_FILTERS or its MPSS_FILTER_* value; widths default to the reference's for the kind;
        params: alpha (gaussian), B and C (mitchell), tau (sinc), the reference's defaults when left out."""
        check(_lib.mpss_set_pixel_filter(self.h, *pixel_filter(kind, xwidth, ywidth, **params)))

    def common_grid(self, mid, near_field=5088):
        """mpss_get_common_grid: the grid the context built for material `mid` and the LDS layout
        near_field, as the dict of mpss.host_common_grid."""
        n = C.c_uint32(0)
        ok = C.c_int()
        check(_lib.mpss_get_common_grid(self.h, mid, int(near_field), None, C.byref(n), *([None] * 11), C.byref(ok)))
        out = dict(rows=np.zeros((n.value, 8), np.float32), bands=np.zeros((8, 4), np.int32),
                   rg=np.zeros(8, np.float32), u0lim=np.zeros(8, np.float32), u1lim=np.zeros(8, np.float32),
                   u1start=np.zeros(8, np.float32), row0=np.zeros(8, np.uint32), ubase=np.zeros(8, np.uint32),
                   rel_err=np.zeros(NB, np.float32), l1_err=np.zeros(NB, np.float32), ua=np.zeros(8, np.float32),
                   hinv=np.zeros(8, np.float32))
        check(_lib.mpss_get_common_grid(self.h, mid, int(near_field), out["rows"].ctypes.data, C.byref(n),
                                        *[out[k].ctypes.data for k in ("bands", "rg", "u0lim", "u1lim", "u1start",
                                                                       "row0", "ubase", "rel_err", "l1_err", "ua",
                                                                       "hinv")], C.byref(ok)))
        out["ok"] = bool(ok.value)
        return out

    def set_material_tables(self, table, rcp, rho_hd, albedo=None, is_mc=False):
        table = np.ascontiguousarray(table, np.float32)
        al = None if albedo is None else np.ascontiguousarray(albedo, np.float32)
        mid = C.c_uint32()
        check(_lib.mpss_set_material_tables(self.h, table, table.shape[1], np.ascontiguousarray(rcp, np.float32),
                                            np.ascontiguousarray(rho_hd, np.float32), len(rho_hd),
                                            None if al is None else al.ctypes.data, int(is_mc), C.byref(mid)))
        return mid.value

    def add_dipole_material(self, sigma_a, sigmap_s, eta):
        """A DiffusionReflectance Rd functor for mo_batch (the dipolesubsurface integrator's Rd)."""
        mid = C.c_uint32()
        check(_lib.mpss_add_dipole_material(self.h, np.ascontiguousarray(sigma_a, np.float32),
                                            np.ascontiguousarray(sigmap_s, np.float32), eta, C.byref(mid)))
        return mid.value

    def material_tables(self, mid):
        L = C.c_uint32()
        nr = C.c_uint32()
        check(_lib.mpss_get_material_tables(self.h, mid, None, C.byref(L), None, None, C.byref(nr), None))
        tab = np.zeros((NB, L.value), np.float32)
        rcp = np.zeros(NB, np.float32)
        rho = np.zeros(nr.value, np.float32)
        tot = np.zeros(NB, np.float32)
        check(_lib.mpss_get_material_tables(self.h, mid, tab.ctypes.data, C.byref(L), rcp.ctypes.data,
                                            rho.ctypes.data, C.byref(nr), tot.ctypes.data))
        return tab, rcp, rho, tot

    def gather_info(self, mid):
        """mpss_get_gather_info: {common_grid: bool, rel_err: (30,), l1_err: (30,)}."""
        on = C.c_int()
        rel = np.zeros(NB, np.float32)
        l1 = np.zeros(NB, np.float32)
        check(_lib.mpss_get_gather_info(self.h, mid, C.byref(on), rel.ctypes.data, l1.ctypes.data))
        return dict(common_grid=bool(on.value), rel_err=rel, l1_err=l1)

    def set_irradiance_points(self, p, n, E, area):
        p, n, E, area = [np.ascontiguousarray(x, np.float32) for x in (p, n, E, area)]
        check(_lib.mpss_set_irradiance_points(self.h, len(p), p, n, E, area))

    def octree_info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(_lib.mpss_octree_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_nodes=a.value, max_depth=b.value, n_points=c.value)

    def octree_export(self):
        """The device octree as the gather reads it (mpss_octree_export): nodes as raw 64-B records
        (np.void), node_et [N, 32], pt_hdr [M, 4], pt_e [M, 32], pt_index [M]."""
        info = self.octree_info()
        N, M = info["n_nodes"], info["n_points"]
        d = dict(nodes=np.zeros((N, 16), np.uint32), node_et=np.zeros((N, 32), np.float32),
                 pt_hdr=np.zeros((M, 4), np.float32), pt_e=np.zeros((M, 32), np.float32),
                 pt_index=np.zeros(M, np.int32))
        check(_lib.mpss_octree_export(self.h, *[d[k].ctypes.data_as(vp) for k in
                                                ("nodes", "node_et", "pt_hdr", "pt_e", "pt_index")]))
        return d

    def mo_batch_paths(self, mid, q, p_dev, mo_dev):
        """mpss_mo_batch_paths: the sharded gather's instrumented pass, its statistics as an (8, 23) uint64
        array (per band group; the slots are listed in include/mpss.h)."""
        stats = np.zeros((8, 23), np.uint64)
        check(_lib.mpss_mo_batch_paths(self.h, mid, q, p_dev, mo_dev, stats.ctypes.data))
        return stats

    def mo_batch(self, mid, q, p_dev, mo_dev, counters_dev=None, stream=None):
        check(_lib.mpss_mo_batch(self.h, mid, q, p_dev, mo_dev, counters_dev, stream))

    # ---- scene slice of the per-pixel path
    def add_mesh(self, P, idx, o2w, w2o, material, N=None, S=None, uv=None, reverse=False):
        P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
        opt = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (N, S, uv)]
        self._keep = opt
        check(_lib.mpss_add_mesh(self.h, len(P), P, *[None if a is None else a.ctypes.data for a in opt],
                                 len(idx), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                 np.ascontiguousarray(o2w, np.float32), np.ascontiguousarray(w2o, np.float32),
                                 int(reverse), material))

    def add_imagemap(self, **tex):
        """Texture "imagemap" (see mpss.imagemap for the keywords); returns its texture id."""
        t, keep = imagemap(**tex)
        tid = C.c_uint32(0)
        check(_lib.mpss_add_imagemap(self.h, C.byref(t), C.byref(tid)))
        del keep
        return tid.value

    def set_material_textures(self, material, albedo=-1, bump=-1):
        check(_lib.mpss_set_material_textures(self.h, material, albedo, bump))

    def set_material_spec_textures(self, material, kr=-1, kt=-1):
        """LayeredSkin's "texture Kr" / "texture Kt": spectrum imagemap ids evaluated per camera hit
        (-1: the material's constant Kr / Kt)."""
        check(_lib.mpss_set_material_spec_textures(self.h, material, kr, kt))

    def add_sphere_light(self, center, radius, Lemit, nsamples=1):
        check(_lib.mpss_add_sphere_light(self.h, np.ascontiguousarray(center, np.float32), radius,
                                         np.ascontiguousarray(Lemit, np.float32), nsamples))

    def add_infinite_light(self, L, nsamples=1, light_to_world=None, world_to_light=None, texels=None):
        """LightSource "infinite"; L = the 30-band L * scale (CreateInfiniteLight); texels = the
        map as an (H, W, 3) float array (ReadImage's RGB), or None for a constant light."""
        l2w = np.eye(4, dtype=np.float32) if light_to_world is None else light_to_world
        w2l = np.linalg.inv(np.asarray(l2w, np.float64)) if world_to_light is None else world_to_light
        args = (self.h, np.ascontiguousarray(L, np.float32), nsamples, np.ascontiguousarray(l2w, np.float32),
                np.ascontiguousarray(w2l, np.float32))
        if texels is None:
            check(_lib.mpss_add_infinite_light(*args))
        else:
            tex = np.ascontiguousarray(texels, np.float32)
            if tex.ndim != 3 or tex.shape[2] != 3:
                raise ValueError("texels must be (height, width, 3)")
            check(_lib.mpss_add_infinite_light_map(*args, tex.shape[1], tex.shape[0], tex))

    def set_camera(self, raster_to_camera, camera_to_world, xres, yres):
        check(_lib.mpss_set_camera(self.h, np.ascontiguousarray(raster_to_camera, np.float32),
                                   np.ascontiguousarray(camera_to_world, np.float32), xres, yres))

    def set_surface_points(self, recs):
        recs = np.ascontiguousarray(recs, SURFACE_POINT)
        check(_lib.mpss_set_surface_points(self.h, len(recs), recs.ctypes.data))

    def surface_points(self):
        n = C.c_uint32()
        check(_lib.mpss_get_surface_points(self.h, None, C.byref(n)))
        out = np.zeros(n.value, SURFACE_POINT)
        check(_lib.mpss_get_surface_points(self.h, out.ctypes.data, C.byref(n)))
        return out

    def load_pointsfile(self, path):
        check(_lib.mpss_load_pointsfile(self.h, os.fsencode(path)))

    def save_pointsfile(self, path):
        check(_lib.mpss_save_pointsfile(self.h, os.fsencode(path)))

    def mc_profile(self, layers, mfp_range=16.0, nsegments=1024, nphotons=100, seed=89, stream=None):
        """Monte-Carlo layered profile; layers: [(mua, musp, ior, thickness), ...]."""
        lay = np.ascontiguousarray(layers, np.float32).reshape(-1, 4)
        r = np.zeros(nsegments, np.float64)
        t = np.zeros(nsegments, np.float64)
        tr, tt, ev = C.c_double(), C.c_double(), C.c_uint64()
        check(_lib.mpss_mc_profile(self.h, lay, len(lay), mfp_range, nsegments, nphotons, seed, r.ctypes.data,
                                   t.ctypes.data, C.byref(tr), C.byref(tt), C.byref(ev), stream))
        return dict(reflectance=r, transmittance=t, total_r=tr.value, total_t=tt.value, events=ev.value)

    def mc_profile_batch(self, layers, mfp_range=16.0, nsegments=1024, nphotons=100, seed=89, rings=True,
                         stream=None):
        """mpss_mc_profile_batch: layers [S, n, 4], every slab traced as mc_profile traces it alone, in one
        kernel launch. rings=False tallies the totals only (reflectance / transmittance are None).
        Arrays carry a leading slab axis; extent [S] is each slab's tally radius; events sums the batch."""
        lay = np.ascontiguousarray(layers, np.float32)
        if lay.ndim != 3 or lay.shape[2] != 4:
            raise ValueError("mc_profile_batch: layers must be [slabs, layers, 4]")
        S, n = lay.shape[0], lay.shape[1]
        r = np.zeros((S, nsegments), np.float64) if rings else None
        t = np.zeros((S, nsegments), np.float64) if rings else None
        tr, tt, ev = np.zeros(S, np.float64), np.zeros(S, np.float64), C.c_uint64()
        check(_lib.mpss_mc_profile_batch(self.h, lay.ctypes.data, S, n, mfp_range, nsegments, nphotons, seed,
                                         r.ctypes.data if rings else None, t.ctypes.data if rings else None,
                                         tr.ctypes.data, tt.ctypes.data, C.byref(ev), stream))
        return dict(reflectance=r, transmittance=t, total_r=tr, total_t=tt, extent=mc_extent(lay, mfp_range),
                    events=ev.value)

    def mc_reference_batch(self, layers, mfp_range=16.0, nsegments=1024, lerp=True, desired_length=1024,
                           max_profiles_per_batch=0, stream=None):
        """mpss_mc_reference_batch: mc_reference for layers [S, n, 4] on the GPU (two-layer slabs; other
        layer counts run the host code per slab). The dict of mc_reference with a leading slab axis."""
        lay = np.ascontiguousarray(layers, np.float32)
        if lay.ndim != 3 or lay.shape[2] != 4:
            raise ValueError("mc_reference_batch: layers must be [slabs, layers, 4]")
        S, n = lay.shape[0], lay.shape[1]
        r = np.zeros((S, nsegments), np.float64)
        t = np.zeros((S, nsegments), np.float64)
        tr, tt = np.zeros(S, np.float64), np.zeros(S, np.float64)
        check(_lib.mpss_mc_reference_batch(self.h, lay.ctypes.data, S, n, mfp_range, nsegments, desired_length,
                                           int(lerp), max_profiles_per_batch, r.ctypes.data, t.ctypes.data,
                                           tr.ctypes.data, tt.ctypes.data, stream))
        return dict(reflectance=r, transmittance=t, total_r=tr, total_t=tt)

    def profile_fit(self, fit, stream=None, timing=False):
        """mpss_profile_fit: fit = profile_fit_spec(...); dict as host_profile_fit, with timing=True also
        stage_ms = (profile stages, fit stages) by HIP events, summed over the batches, and batches = how many
        batches of profiles ran."""
        f = fit[0]
        ms = (C.c_double * 3)()
        out = _profile_fit_call(lambda ns, ni, s, c, e, r, ce: _lib.mpss_profile_fit(
            self.h, C.byref(f), C.byref(ns), C.byref(ni), s, c, e, r, ce, C.addressof(ms) if timing else None,
            stream))
        if timing:
            out["stage_ms"] = (ms[0], ms[1])
            out["batches"] = int(ms[2])
        return out

    def sog_fit(self, dist_sq, data, sigmas, mfp_min, mfp_max, stream=None):
        """mpss_sog_fit: the fit stage alone on host arrays (see host_sog_fit)."""
        args, out = _sog_args(dist_sq, data, sigmas, mfp_min, mfp_max)
        check(_lib.mpss_sog_fit(self.h, *args, out["coeffs"].ctypes.data, out["error"].ctypes.data,
                                out["centre"].ctypes.data, out["cand_error"].ctypes.data,
                                out["cand_coeffs"].ctypes.data, stream))
        return out

    def replay_samples(self, spp, xres, yres):
        """The reference sampler's values over the sample extent: (yres+1, xres+1, spp', K) float32."""
        n, k = C.c_uint64(), C.c_int()
        check(_lib.mpss_replay_samples(self.h, spp, None, C.byref(n), C.byref(k)))
        out = np.zeros(n.value, np.float32)
        check(_lib.mpss_replay_samples(self.h, spp, out.ctypes.data, C.byref(n), C.byref(k)))
        return out.reshape(yres + 1, xres + 1, -1, k.value)

    def irradiance(self):
        n = C.c_uint32()
        check(_lib.mpss_get_irradiance(self.h, None, C.byref(n)))
        out = np.zeros((n.value, NB), np.float32)
        check(_lib.mpss_get_irradiance(self.h, out.ctypes.data, C.byref(n)))
        return out

    def render_stats(self):
        st = RenderStats()
        check(_lib.mpss_get_render_stats(self.h, C.byref(st)))
        out = {}
        for k, _ in RenderStats._fields_:
            v = getattr(st, k)
            out[k] = [list(x) for x in v] if k == "group_bands" or k.startswith("group_path") else (
                list(v) if k.startswith("group_") or k == "mo_lookups_near" else v)
        return out

    def set_instrumentation(self, kernel_timing=False, count_traversal=False):
        """count_traversal: False/0, True/1 (the gather's own visits), or 2 (the reference
        traversal's visits: reach pruning off, results unchanged)."""
        check(_lib.mpss_set_instrumentation(self.h, int(kernel_timing), int(count_traversal)))

    def reset_render_stats(self):
        check(_lib.mpss_reset_render_stats(self.h))

    def preprocess(self, seed=0):
        check(_lib.mpss_preprocess(self.h, seed))

    def render_tile(self, spp, seed, x0, x1, y0, y1, out_dev, stream=None):
        check(_lib.mpss_render_tile(self.h, spp, seed, x0, x1, y0, y1, out_dev, stream))

    def tile_costs(self, rects):
        """Per rectangle (x0, x1, y0, y1): camera rays through pixel centres that hit a BSSRDF
        surface, and that hit any mesh (mpss_tile_costs) -> two int64 arrays."""
        n = len(rects)
        r = (C.c_int32 * (4 * max(n, 1)))(*[int(v) for rc in rects for v in rc])
        sss = np.zeros(max(n, 1), np.int64)
        surf = np.zeros(max(n, 1), np.int64)
        check(_lib.mpss_tile_costs(self.h, n, r, sss.ctypes.data, surf.ctypes.data))
        return sss[:n], surf[:n]

    def render_tiles(self, spp, seed, rects, outs_dev, stream=None):
        """rects: [(x0, x1, y0, y1)], outs_dev: device pointers (one float4 XYZW tile each)."""
        n = len(rects)
        r = (C.c_int32 * (4 * n))(*[int(v) for rc in rects for v in rc])
        o = (vp * n)(*outs_dev)
        check(_lib.mpss_render_tiles(self.h, spp, seed, n, r, o, stream))

    def render_tile_spectral(self, spp, seed, x0, x1, y0, y1, spec_dev, out_dev=None, stream=None):
        """mpss_render_tile_spectral: spec_dev receives SPECTRAL_ROW floats per pixel (30 band sums, the weight
        sum, 0); out_dev (optional) the XYZW tile render_tile writes."""
        check(_lib.mpss_render_tile_spectral(self.h, spp, seed, x0, x1, y0, y1, spec_dev, out_dev, stream))

    def render_tiles_spectral(self, spp, seed, rects, specs_dev, outs_dev=None, stream=None):
        """rects: [(x0, x1, y0, y1)]; specs_dev: device pointers (SPECTRAL_ROW floats per pixel each);
        outs_dev: None, or one XYZW device pointer (or None) per rectangle."""
        n = len(rects)
        r = (C.c_int32 * (4 * max(n, 1)))(*[int(v) for rc in rects for v in rc])
        s = (vp * max(n, 1))(*specs_dev)
        o = None if outs_dev is None else (vp * max(n, 1))(*outs_dev)
        check(_lib.mpss_render_tiles_spectral(self.h, spp, seed, n, r, s, o, stream))
