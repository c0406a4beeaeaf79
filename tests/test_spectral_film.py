"""The spectral film's host side (CPU only): mpss_host_spectrum_to_xyz against the oracle's ToXYZ, the cube's
EXR writer and channel reader, finalize_spectral, and the new entry points of the C ABI."""
import subprocess

import numpy as np

import synth

NB = 30


def _oracle_xyz(oracle, spectra):
    out = np.zeros((len(spectra), 3), np.float32)
    for i, s in enumerate(spectra):
        oracle.lib().o_to_xyz(np.ascontiguousarray(s, np.float32), out[i])
    return out


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_to_xyz_unit_spectra_bit_exact(mpss, oracle):
    e = np.eye(NB, dtype=np.float32)
    got = mpss.host_spectrum_to_xyz(e)
    assert got.shape == (NB, 3) and np.all(got >= 0) and got.max() > 0
    assert _same_bits(got, _oracle_xyz(oracle, e))


def test_to_xyz_smooth_spectra_bit_exact(mpss, oracle):
    s = synth.smooth_spectra(64)
    assert _same_bits(mpss.host_spectrum_to_xyz(s), _oracle_xyz(oracle, s))
    # the leading axes are kept
    assert _same_bits(mpss.host_spectrum_to_xyz(s.reshape(8, 8, NB)).reshape(64, 3), _oracle_xyz(oracle, s))


def test_to_xyz_applies_no_sample_filter(mpss, oracle):
    """A NaN band and a negative band go through the sums as they are: rejecting a sample is the renderer's
    business (SamplerRenderer), not ToXYZ's."""
    s = synth.smooth_spectra(2, seed=5)
    s[0, 7] = np.nan
    s[1, 14] = -100.0
    got = mpss.host_spectrum_to_xyz(s)
    assert _same_bits(got, _oracle_xyz(oracle, s))
    assert np.all(np.isnan(got[0]))
    pos = s[1].copy()
    pos[14] = 0.0
    assert got[1, 1] < mpss.host_spectrum_to_xyz(pos)[1] and got[1, 1] < -1e-5


def test_spectral_exr_round_trip(mpss, tmp_path):
    from mpss import film, imageio
    rng = np.random.default_rng(3)
    cube = rng.standard_normal((5, 7, NB)).astype(np.float32) * np.float32(1e3)
    cube[0, 0, 0] = np.float32(1e-30)  # no HALF channel holds these two
    cube[4, 6, 29] = np.float32(3e38)
    for comp in ("zip", "none"):
        path = str(tmp_path / ("cube_%s.exr" % comp))
        film.write_spectral_exr(path, cube, compression=comp)
        planes = imageio.read_exr_channels(path)
        names = list(planes)
        assert names == ["S0.%dnm" % nm for nm in range(405, 700, 10)] == film.spectral_channel_names()
        assert names == sorted(names)  # the file's channel order is the wavelength order
        assert film.band_centres() == list(range(405, 700, 10))
        for c, nm in enumerate(names):
            assert planes[nm].dtype == np.float32 and _same_bits(planes[nm], np.ascontiguousarray(cube[..., c]))
    # FLOAT channels in the header: pixel type 2 after every name
    raw = open(path, "rb").read()
    i = raw.index(b"S0.405nm\0")
    assert int.from_bytes(raw[i + 9:i + 13], "little") == 2


def test_read_exr_rgb_unchanged(mpss, tmp_path):
    """read_exr on a file written by write_exr: the half-rounded R, G, B as before read_exr_channels was
    factored out of it, and the channels it is made of."""
    from mpss import film, imageio
    rng = np.random.default_rng(4)
    rgb = rng.random((19, 6, 3), dtype=np.float32) * np.float32(4)
    path = str(tmp_path / "rgb.exr")
    film.write_exr(path, rgb)
    got = imageio.read_exr(path)
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
    assert _same_bits(got, rgb.astype(np.float16).astype(np.float32))
    planes = imageio.read_exr_channels(path)
    assert list(planes) == ["A", "B", "G", "R"] and np.all(planes["A"] == 1)
    assert _same_bits(np.stack([planes["R"], planes["G"], planes["B"]], -1), got)


def test_finalize_spectral(mpss):
    from mpss import film
    rng = np.random.default_rng(5)
    spec = np.zeros((3, 4, 32), np.float32)
    spec[..., :30] = rng.random((3, 4, 30), dtype=np.float32)
    spec[..., 30] = np.float32(8)
    spec[1, 2, :31] = 0  # no sample reached this pixel: weight 0 gives 0, not NaN
    spec[2, 3, 30] = np.float32(-0.25)  # a negative weight sum (mitchell) still divides
    cube = film.finalize_spectral(spec)
    assert cube.shape == (3, 4, 30) and cube.dtype == np.float32
    assert np.all(cube[1, 2] == 0) and not np.isnan(cube).any()
    with np.errstate(divide="ignore"):
        inv = np.float32(1) / spec[..., 30:31].astype(np.float32)
    want = (spec[..., :30] * np.where(spec[..., 30:31] != 0, inv, 1)).astype(np.float32)
    assert _same_bits(cube, want)
    # the same rule as finalize's weight division: one band alone in X, Y, Z
    assert np.array_equal(cube[0, 0], spec[0, 0, :30] * (np.float32(1) / np.float32(8)))


def test_abi_exports_spectral_entry_points(mpss):
    assert mpss.lib().mpss_abi_version() == 13  # new entry points are found by symbol, not by version
    new = ["mpss_render_tile_spectral", "mpss_render_tiles_spectral", "mpss_host_spectrum_to_xyz"]
    declared = mpss.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", mpss.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in new:
        assert s in declared and s in exported
        assert getattr(mpss.lib(), s).argtypes is not None  # mirrored in the binding
    assert mpss.SPECTRAL_ROW == 32
    # null arguments fail with a message, before a context or a device is touched
    assert mpss.lib().mpss_render_tile_spectral(None, 1, 0, 0, 1, 0, 1, None, None, None) == -1
    assert b"null" in mpss.lib().mpss_last_error()
    assert mpss.lib().mpss_host_spectrum_to_xyz.restype is not None
