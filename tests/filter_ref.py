"""numpy restatement of the reference's pixel filters and film, for the pixel-filter tests.

  - the five Filter::Evaluate functions (filters/{box,triangle,gaussian,mitchell,sinc}.{h,cpp}) and
    ImageFilm's 16 x 16 filterTable (film/image.cpp:56-68), in float32 operation for operation;
  - ImageFilm::AddSample (image.cpp:77-137) and GetSampleExtent (image.cpp:157-166);
  - the counter-hash sampler's image positions (hash3 / mix32 of csrc/pbrt_math.h, van der Corput and
    Sobol' as in tests/test_sampler_replay.py), with the key of pixels outside the frame:
    xres * yres + (py - ys) * (xe - xs) + (px - xs) over the sample extent [xs, xe) x [ys, ye).

Sums are accumulated in float64; weights, positions and indices are float32 as in the reference.
"""
import numpy as np

F = np.float32
KINDS = ("box", "triangle", "gaussian", "mitchell", "sinc")
# (xwidth, ywidth, a, b) of core/api.cpp's Create*Filter; a, b: alpha | B, C | tau
DEFAULTS = {"box": (0.5, 0.5, 0.0, 0.0), "triangle": (2.0, 2.0, 0.0, 0.0), "gaussian": (2.0, 2.0, 2.0, 0.0),
            "mitchell": (2.0, 2.0, 1.0 / 3.0, 1.0 / 3.0), "sinc": (4.0, 4.0, 3.0, 0.0)}
ONE_M_EPS = F(float.fromhex("0x1.fffffep-1"))
TABLE = 16


def describe(kind, xwidth=None, ywidth=None, a=None, b=None):
    """(kind index, xwidth, ywidth, a, b) as float32, the reference's defaults filled in."""
    d = DEFAULTS[kind]
    v = [d[i] if x is None else x for i, x in enumerate((xwidth, ywidth, a, b))]
    return (KINDS.index(kind), F(v[0]), F(v[1]), F(v[2]), F(v[3]))


def _gaussian1d(alpha, d, expv):
    return max(F(0), F(np.exp(F(F(-alpha) * d * d)) - expv))


def _mitchell1d(B, C, x):
    x = abs(F(2) * x)
    s = F(F(1) / F(6))
    k = lambda v: F(v)  # the reference's integer constants, converted to float before each product
    if x > F(1):
        return F(((-B - k(6) * C) * x * x * x + (k(6) * B + k(30) * C) * x * x + (k(-12) * B - k(48) * C) * x +
                  (k(8) * B + k(24) * C)) * s)
    return F(((k(12) - k(9) * B - k(6) * C) * x * x * x + (k(-18) + k(12) * B + k(6) * C) * x * x +
              (k(6) - k(2) * B)) * s)


def _sinc1d(tau, x):
    x = abs(x)
    if float(x) < 1e-5:
        return F(1)
    if float(x) > 1.0:
        return F(0)
    x = F(float(x) * np.pi)
    sinc = F(np.sin(x) / x)
    lanczos = F(np.sin(F(x * tau)) / F(x * tau))
    return F(sinc * lanczos)


def evaluate(f, x, y):
    kind, xw, yw, a, b = f
    x, y = F(x), F(y)
    name = KINDS[kind]
    if name == "box":
        return F(1)
    if name == "triangle":
        return F(max(F(0), xw - abs(x)) * max(F(0), yw - abs(y)))
    if name == "gaussian":
        ex, ey = F(np.exp(F(F(-a) * xw * xw))), F(np.exp(F(F(-a) * yw * yw)))
        return F(_gaussian1d(a, x, ex) * _gaussian1d(a, y, ey))
    ix, iy = F(F(1) / xw), F(F(1) / yw)
    if name == "mitchell":
        return F(_mitchell1d(a, b, F(x * ix)) * _mitchell1d(a, b, F(y * iy)))
    return F(_sinc1d(a, F(x * ix)) * _sinc1d(a, F(y * iy)))


def table(f):
    """filterTable, [256] float32: entry 16 y + x."""
    _, xw, yw, _, _ = f
    t = np.zeros(TABLE * TABLE, F)
    for y in range(TABLE):
        fy = F(F(F(y) + F(.5)) * yw / F(TABLE))
        for x in range(TABLE):
            fx = F(F(F(x) + F(.5)) * xw / F(TABLE))
            t[y * TABLE + x] = evaluate(f, fx, fy)
    return t


def sample_extent(f, xres, yres):
    _, xw, yw, _, _ = f
    return (int(np.floor(F(F(0.5) - xw))), int(np.ceil(F(F(F(0.5) + F(xres)) + xw))),
            int(np.floor(F(F(0.5) - yw))), int(np.ceil(F(F(F(0.5) + F(yres)) + yw))))


def halo(width):
    return int(np.ceil(F(F(width) + F(0.5))))


def pixel_range(X, w, res):
    """AddSample's clamped [x0, x1] of float32 coordinates X (arrays)."""
    d = (np.asarray(X, F) - F(0.5)).astype(F)
    lo = np.ceil((d - F(w)).astype(F)).astype(np.int64)
    hi = np.floor((d + F(w)).astype(F)).astype(np.int64)
    return np.maximum(lo, 0), np.minimum(hi, res - 1)


def table_index(x, X, w):
    """ifx of pixel(s) x for float32 coordinate(s) X."""
    d = (np.asarray(X, F) - F(0.5)).astype(F)
    inv = F(F(1) / F(w))
    fx = np.abs(((np.asarray(x).astype(F) - d).astype(F) * inv).astype(F) * F(TABLE)).astype(F)
    return np.minimum(np.floor(fx).astype(np.int64), TABLE - 1)


# ---------------------------------------------------------------- the hash sampler's image samples
def _mix32(h):
    h = h & 0xffffffff
    h ^= h >> 16
    h = (h * 0x7feb352d) & 0xffffffff
    h ^= h >> 15
    h = (h * 0x846ca68b) & 0xffffffff
    h ^= h >> 16
    return h


def hash3(a, b, c):
    """mix32(a ^ mix32(b ^ mix32(c + 0x9e3779b9))) on uint64 arrays holding 32-bit values."""
    a, b, c = (np.asarray(v, np.uint64) for v in (a, b, c))
    return _mix32(a ^ _mix32(b ^ _mix32((c + np.uint64(0x9e3779b9)) & np.uint64(0xffffffff))))


def _unit(bits):
    return np.minimum(((bits >> np.uint64(8)) & np.uint64(0xffffff)).astype(F) / F(1 << 24), ONE_M_EPS)


def vdc(n, scr):
    r = int("{:032b}".format(int(n) & 0xffffffff)[::-1], 2)
    return _unit(np.asarray(scr, np.uint64) ^ np.uint64(r))


def sobol2(n, scr):
    v, m = 1 << 31, 0
    n = int(n)
    while n:
        if n & 1:
            m ^= v
        n >>= 1
        v ^= v >> 1
    return _unit(np.asarray(scr, np.uint64) ^ np.uint64(m))


def pixel_keys(f, xres, yres):
    """(px, py, key) over the sample extent, each [eh, ew]."""
    xs, xe, ys, ye = sample_extent(f, xres, yres)
    py, px = np.mgrid[ys:ye, xs:xe]
    inside = (px >= 0) & (px < xres) & (py >= 0) & (py < yres)
    key = np.where(inside, py * xres + px, xres * yres + (py - ys) * (xe - xs) + (px - xs))
    return px, py, key.astype(np.uint64) & np.uint64(0xffffffff)


def image_positions(f, xres, yres, spp, seed):
    """(px, py, X, Y): pixels [eh, ew] of the sample extent and their samples' float32 image positions
    [eh, ew, spp] (imageX = x + u in float)."""
    px, py, key = pixel_keys(f, xres, yres)
    s0, s1 = hash3(np.uint64(seed), key, np.uint64(0)), hash3(np.uint64(seed), key, np.uint64(1))
    X = np.stack([px.astype(F) + vdc(s, s0) for s in range(spp)], -1).astype(F)
    Y = np.stack([py.astype(F) + sobol2(s, s1) for s in range(spp)], -1).astype(F)
    return px, py, X, Y


def add_samples(f, xres, yres, X, Y, xyz=None):
    """ImageFilm::AddSample of every sample (X, Y: float32, any shape; xyz: matching [..., 3] or None
    for weights alone). Returns float64 dict: film [yres, xres, 4] (sum w x, sum w), absw = sum |w|,
    absx [yres, xres, 3] = sum |w x|, n = contributing samples per pixel."""
    _, xw, yw, _, _ = f
    tab = table(f).astype(np.float64)
    X, Y = np.asarray(X, F).ravel(), np.asarray(Y, F).ravel()
    x3 = None if xyz is None else np.asarray(xyz, np.float64).reshape(-1, 3)
    lx, hx = pixel_range(X, xw, xres)
    ly, hy = pixel_range(Y, yw, yres)
    film = np.zeros((yres, xres, 4))
    absw, n, absx = np.zeros((yres, xres)), np.zeros((yres, xres), np.int64), np.zeros((yres, xres, 3))
    for oy in range(int((hy - ly).max()) + 1):
        y = ly + oy
        for ox in range(int((hx - lx).max()) + 1):
            x = lx + ox
            ok = (y <= hy) & (x <= hx)
            if not ok.any():
                continue
            xo, yo = x[ok], y[ok]
            w = tab[table_index(yo, Y[ok], yw) * TABLE + table_index(xo, X[ok], xw)]
            np.add.at(film[..., 3], (yo, xo), w)
            np.add.at(absw, (yo, xo), np.abs(w))
            np.add.at(n, (yo, xo), 1)
            if x3 is not None:
                for c in range(3):
                    np.add.at(film[..., c], (yo, xo), w * x3[ok, c])
                    np.add.at(absx[..., c], (yo, xo), np.abs(w * x3[ok, c]))
    return dict(film=film, absw=absw, absx=absx, n=n)
