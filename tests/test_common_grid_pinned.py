"""The common grid the host builder makes (csrc/common_grid.cpp build_common_grid, through
mpss.host_common_grid), pinned bit for bit: for each case below and each LDS layout, a SHA-256 over the
uint32 views of every field tests/test_common_grid_gpu.py compares (FIELDS) and `ok` must equal the
one in tests/golden/common_grid_pins.json. The fixture was written once by tools/make_common_grid_pins.py
from the library as it stood before the builder became its own unit (and lost its sparse-table range
search); whatever is built since must reproduce it -- the range choice included: a different range on
any of these inputs is a bug.

The cases are the smallest tables that reach each branch of the builder. They are made only of
IEEE-exact operations (+ - * /), np.random.default_rng(seed).random and the committed
tests/golden/golden.npz profile -- no exp or pow, whose last bit differs between numpy builds -- so the
inputs are the same bytes on any machine. `reaches` names what the generator checked of each case
on the library that wrote the fixture.
"""
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden.npz")
PINS = os.path.join(ROOT, "tests", "golden", "common_grid_pins.json")
NEAR_FIELDS = (5088, 10236)
FIELDS = ("rows", "bands", "rg", "u0lim", "u1lim", "u1start", "row0", "ubase", "rel_err", "l1_err", "ua", "hinv")


def _decay(L, rate, power=1):
    """1 / (1 + rate_c x)^(2^power) on x = k / L: a smooth decay from exact operations (squared `power` times)."""
    x = np.arange(L, dtype=np.float64) / L
    y = 1.0 / (1.0 + np.asarray(rate, np.float64)[:, None] * x[None, :])
    for _ in range(power):
        y = y * y
    return y


def _spread_rcp(L, lo, hi):
    """rcpDsqSpacing of 30 bands whose reaches spread from lo to hi"""
    reach = lo + (hi - lo) * np.arange(30, dtype=np.float64) / 29.0
    return ((L - 1) / reach).astype(np.float32)


def _case(name):
    """(table [30][L] float32, rcp [30] float32, keyword arguments of mpss.host_common_grid)"""
    c = np.arange(30, dtype=np.float64)
    if name == "L3":  # too short: declines
        return np.ones((30, 3), np.float32), np.full(30, 100.0, np.float32), {}
    if name == "L4":  # the shortest table that is looked at
        return _decay(4, 4 + 0.2 * c).astype(np.float32), np.full(30, 3.0 / 0.004, np.float32), {}
    if name == "zero_rcp":  # a band without a spacing: declines
        rcp = np.full(30, 99.0 / 0.004, np.float32)
        rcp[7] = 0.0
        return _decay(100, 4 + 0.2 * c).astype(np.float32), rcp, {}
    if name == "rough":  # 30 % noise on a steep decay: flagged cells, more bad fine knots than range starts
        L = 4096
        noise = 1.0 + 0.3 * np.random.default_rng(5).random((30, L))
        return (_decay(L, 3 + c, 5) * noise).astype(np.float32), _spread_rcp(L, 0.01, 1.0), {}
    if name == "equal":  # one spacing for all bands: the rows are the tables
        L = 30000
        return _decay(L, 4 + 0.2 * c).astype(np.float32), np.full(30, (L - 1) / 0.004, np.float32), {}
    if name in ("smooth", "smooth_snake"):  # spread spacings, fine rows to the end (H = 1)
        L = 6000
        return _decay(L, 5 + 0.3 * c).astype(np.float32), _spread_rcp(L, 0.002, 0.006), dict(snake=name == "smooth_snake")
    if name == "rgb":  # rgbprofile: rows 0..2 in every group, 28 floats of the LDS reserved
        L = 6000
        return _decay(L, 5 + 3.0 * c).astype(np.float32), _spread_rcp(L, 0.006, 0.002), dict(rgb=True)
    if name == "coarse":  # long and smooth: the row cap binds and some group's rows go H > 1 steps apart
        L = COARSE_L
        return _decay(L, 5 + 0.3 * c).astype(np.float32), _spread_rcp(L, 0.002, 0.006), {}
    if name == "golden":  # the committed desiredlength-64 skin profile
        z = np.load(GOLDEN)
        return z["profile_64"], z["profile_64_rcp"], {}
    raise KeyError(name)


COARSE_L = 60000  # (56000: H > 1 for the 5088 layout only; 52000: for neither)
CASES = ("L3", "L4", "zero_rcp", "rough", "equal", "smooth", "smooth_snake", "rgb", "coarse", "golden")


def grid_hash(cg):
    h = hashlib.sha256()
    h.update(b"ok1" if cg["ok"] else b"ok0")
    for k in FIELDS:
        a = np.ascontiguousarray(cg[k])
        h.update(("%s%r" % (k, a.shape)).encode())
        h.update(a.view(np.uint32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("near_field", NEAR_FIELDS)
@pytest.mark.parametrize("name", CASES)
def test_pinned_grid(mpss, name, near_field):
    with open(PINS) as f:
        pins = json.load(f)
    tab, rcp, kw = _case(name)
    cg = mpss.host_common_grid(tab, rcp, near_field=near_field, **kw)
    want = pins["%s/%d" % (name, near_field)]
    assert cg["ok"] == want["ok"], (name, near_field)
    assert grid_hash(cg) == want["sha256"], (name, near_field, want["reaches"])
