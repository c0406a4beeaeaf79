"""Synthetic skin textures for scenes/skin_textured.pbrt and scenes/skin_spec.pbrt (the fork's S007
scene drives LayeredSkin's "albedo" and "bumpmap" with imagemaps, scenes/BasicMeshScenes/
S007Scene.pbrt:31-34,49-50, and its GTRenders/GT00x...SpecTex scenes "Kr"; the image files are not
in the reference snapshot). Deterministic: value noise of fixed seeds.

    python tools/make_textures.py   -> scenes/textures/skin_albedo.tga, skin_bump.tga and
                                       tests/golden/skin_spec.tga

(the repository keeps new binary files under tests/golden/ only; scenes/skin_spec.pbrt names the map
there, and tests/test_spec_texture.py holds the tracked files to these generators byte for byte.)

albedo: 512x512 RGB, a pale skin tone modulated by low-frequency blotches and small freckles;
bump: 256x256 grey, pores / fine wrinkles (the float imagemap takes the texel's average);
spec: 256x256 RGB, a faintly warm specular level (about 0.55-0.85, which "gamma" 2.2 "scale" 2 takes
to about 0.5-1.4) with every fourth 32x32 cell exactly black -- no Microfacet lobe at those hits.
All 8-bit uncompressed TGA (ReadImageTGA, imageio.cpp:214-256). The spec map has a generator and a
seed of its own, so the other two files do not depend on it."""
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def value_noise(n, cells, rng):
    g = rng.random((cells + 1, cells + 1))
    x = np.linspace(0, cells, n, endpoint=False)
    i = x.astype(int)
    f = x - i
    f = f * f * (3 - 2 * f)
    a = g[i][:, i] * (1 - f)[None, :] + g[i][:, i + 1] * f[None, :]
    b = g[i + 1][:, i] * (1 - f)[None, :] + g[i + 1][:, i + 1] * f[None, :]
    return a * (1 - f)[:, None] + b * f[:, None]


def fbm(n, rng, octaves):
    out = np.zeros((n, n))
    amp, tot = 1.0, 0.0
    for o in range(octaves):
        out += amp * value_noise(n, 4 << o, rng)
        tot += amp
        amp *= 0.5
    return out / tot


def tga_bytes(rgb8):
    h, w, _ = rgb8.shape
    hdr = struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, w, h, 24, 0x20)  # top-left origin
    return hdr + np.ascontiguousarray(rgb8[..., ::-1]).tobytes()


def write_tga(path, rgb8):
    with open(path, "wb") as f:
        f.write(tga_bytes(rgb8))


def albedo_and_bump():
    """skin_albedo.tga and skin_bump.tga as (H, W, 3) uint8 arrays (one random stream, in this order)."""
    rng = np.random.default_rng(0x5EED)
    n = 512
    base = np.array([0.80, 0.62, 0.52])
    blot = fbm(n, rng, 5)
    freck = np.clip((fbm(n, rng, 7) - 0.62) * 6.0, 0, 1)
    alb = base[None, None, :] * (0.85 + 0.3 * blot[..., None]) * (1 - 0.35 * freck[..., None] * np.array([0.5, 0.8, 0.9]))
    alb8 = np.clip(np.round(alb * 255), 0, 255).astype(np.uint8)
    m = 256
    bump = 0.5 + 0.35 * (fbm(m, rng, 6) - 0.5) + 0.15 * (value_noise(m, 96, rng) - 0.5)
    g = np.clip(np.round(bump * 255), 0, 255).astype(np.uint8)
    return alb8, np.repeat(g[..., None], 3, axis=2)


def spec():
    """skin_spec.tga as a (256, 256, 3) uint8 array."""
    rng = np.random.default_rng(0x5BEC)
    n, cell = 256, 32
    level = 0.55 + 0.3 * fbm(n, rng, 5)
    rgb = level[..., None] * np.array([1.0, 0.97, 0.94])
    i = np.arange(n) // cell
    rgb[(i[:, None] + i[None, :]) % 4 == 0] = 0.0  # (rows x columns of cells: 16 of the 64)
    return np.clip(np.round(rgb * 255), 0, 255).astype(np.uint8)


def main(out_dir=None, spec_dir=None):
    out_dir = out_dir or os.path.join(ROOT, "scenes", "textures")
    spec_dir = spec_dir or os.path.join(ROOT, "tests", "golden")
    alb8, bump8 = albedo_and_bump()
    write_tga(os.path.join(out_dir, "skin_albedo.tga"), alb8)
    write_tga(os.path.join(out_dir, "skin_bump.tga"), bump8)
    write_tga(os.path.join(spec_dir, "skin_spec.tga"), spec())


if __name__ == "__main__":
    main()
