#!/usr/bin/env python3
"""Writes tests/golden/common_grid_pins.json: the hashes tests/test_common_grid_pinned.py holds the host
grid builder to. Run it against the library whose grids are to be pinned (MPSS_LIB=path/to/libmpss.so
for another build than the tree's). Each case must reach its branch on that library before its hash is
written; the check's wording goes into the fixture as `reaches`.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v2-skin_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bad_fine_cells(tab, rcp, cg, g):
    """Distinct fine cells of group g holding a band knot off by more than the bound (the H = 1 per-knot
    test restated in numpy: a count, not bit for bit)."""
    from test_common_grid import ABS_TOL, _R
    L = tab.shape[1]
    T = tab.astype(np.float64)
    cells = set()
    for c in cg["bands"][g]:
        if c < 0:
            continue
        r = np.float64(rcp[c]) / np.float64(cg["rg"][g])
        k = np.arange(max(0, int(np.floor(float(cg["u0lim"][g]) * r)) - 1), L - 1)
        u = k / r
        m = np.floor(u)
        approx = (1 - (u - m)) * _R(T[c], r, m, L).astype(np.float32) + (u - m) * _R(T[c], r, m + 1, L).astype(np.float32)
        over = np.abs(approx - T[c, k]) > np.maximum(2e-6 * np.abs(T[c, k]), ABS_TOL * np.abs(T[c]).max())
        cells |= set(m[over].astype(int).tolist())
    return len(cells)


def reaches(name, cg, tab, rcp):
    """The branch the case is there for, checked on this library's grid; returns its description."""
    rows, nan = cg["rows"], np.isnan(cg["rows"][:, 0])
    if name in ("L3", "zero_rcp"):
        assert not cg["ok"] and len(rows) == 0
        return "declines: no rows"
    if name == "L4":
        assert float(cg["u0lim"].min()) > 0
        return "the LDS split is made"
    assert cg["ok"]
    if name == "rough":
        # flagged cells, and in a group that has rows more bad fine knots than the 64 starts tried
        most = max(bad_fine_cells(tab, rcp, cg, g) for g in range(8) if cg["u1lim"][g] > cg["u0lim"][g])
        assert nan.any() and most > 64
        return "%d flagged cells; %d distinct bad fine knots in one group with rows (> 64 starts)" % (int(nan.sum()), most)
    if name == "equal":
        assert float(cg["rel_err"].max()) == 0.0
        return "rel_err 0: the rows are the tables"
    if name in ("smooth", "smooth_snake"):
        assert float(cg["hinv"].min()) == 1.0 and len(set(cg["rg"].tolist())) == 8
        return "eight grids, every group H = 1"
    if name == "rgb":
        assert np.all(cg["bands"] == np.array([0, 1, 2, -1])) and len(set(cg["u1lim"].tolist())) == 1
        return "slots 0..2 in every group, one grid copied"
    if name == "coarse":
        n = np.diff(np.append(cg["row0"], len(rows)))
        assert float(cg["hinv"].min()) < 1.0 and int(n.max()) > 49152 - 64  # (ua steps by 64)
        return "hinv.min() = %g, %d rows in one group (the cap: 49152)" % (float(cg["hinv"].min()), int(n.max()))
    if name == "golden":
        return "ok"
    raise KeyError(name)


def main():
    import mpss
    import test_common_grid_pinned as t

    pins = {}
    for name in t.CASES:
        tab, rcp, kw = t._case(name)
        for nf in t.NEAR_FIELDS:
            cg = mpss.host_common_grid(tab, rcp, near_field=nf, **kw)
            pins["%s/%d" % (name, nf)] = dict(ok=bool(cg["ok"]), reaches=reaches(name, cg, tab, rcp), sha256=t.grid_hash(cg))
            print(name, nf, pins["%s/%d" % (name, nf)]["reaches"])
    with open(t.PINS, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
