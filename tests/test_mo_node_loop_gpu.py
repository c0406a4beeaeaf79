"""The sharded gather's node and leaf loops, pinned bit for bit.

A change to how the walk forms its lane masks, keeps its wave-uniform state or schedules its
instructions must not change a sum: tests/golden/mo_node_loop_small.npz holds mpss_mo_batch's
outputs and per-query visit counters for one small seeded case, recorded from the build before the
node test was rewritten as lane masks, and every variant below must reproduce them exactly.

The case: 6000 seeded points on an ellipsoid (5 % black and a black cap, so leaves have odd live counts
and black subtrees occur), a 16384-entry synthetic profile (longer than both near fields, with a different
reach per band, so subtrees are pruned per group and all 8 band groups are non-empty), 200 queries
-- three full waves and one of 8 live lanes whose other 56 entries of the permutation are -1 --
on the surface, at a point (d2 = 0), inside the root box away from the surface and far outside it.
Variants: the common grid with the 5088- and the 10236-entry near field, the per-band tables, and the
rgbprofile family once (an rgbprofile LayeredSkin on the same cloud, shrunk to its profiles' reach).

Coverage is asserted from the kernel's own counters: mpss_mo_batch_paths runs the instrumented pass over
the case and returns its lane-record and path counters, and each of these must be non-zero -- the LDS,
row and own-table paths, a flagged row cell, a leaf that qualifies for the LDS-only pair loop (the loop
itself is compiled into the uninstrumented kernel only, whose sums the golden pins), a leaf with an odd
live count, a pruned subtree, a black node, and a query inside the box of a node other than the root.
"""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mo_node_loop_small.npz")
RADII = (0.05, 0.06, 0.07)
L = 16384
EXTENT = 0.004  # d2 at band 0's profile end
MAX_ERROR = 0.1
VARIANTS = {"cg_5088": dict(), "cg_10236": dict(mo_near_field=10236), "bands_5088": dict(mo_common_grid=0),
            "rgb_cg_5088": dict(rgb=True)}
# the rgbprofile family's material (tests/test_rgbprofile_gpu.py's skin) and the scale of its patch
RGB_SKIN = dict(roughness=0.3, nmperunit=40e6, f_mel=0.5, f_eu=0.5, f_blood=0.5, f_ohg=0.5,
                layer_thickness_nm=(0.25e6, 20e6), layer_ior=(1.4, 1.4))
RGB_SCALE = 0.1  # the case's ellipsoid (radii 0.05-0.07) shrunk to a few profile reaches across


def case():
    x = np.linspace(0, 1, L, dtype=np.float32)
    table = np.stack([(np.exp(-x * (4 + 0.2 * c)) * (1 + 0.01 * c)).astype(np.float32) for c in range(30)])
    rcp = np.array([(L - 1) / (EXTENT * (1 + 0.03 * c)) for c in range(30)], np.float32)
    p, n, E, area = synth.ellipsoid_cloud(6000, radii=RADII, seed=41, black_frac=0.05)
    E = E.copy()
    E[p[:, 0] > 0.8 * RADII[0]] = 0  # a cap without irradiance: whole subtrees are black nodes
    cloud = (p, n, E, area)
    q = np.concatenate([synth.surface_queries(196, radii=RADII, seed=43),
                        cloud[0][:2],                                  # on a point: d2 = 0
                        np.float32([[0.0, 0.0, 0.0]]),                 # inside the root box, far from every point
                        np.float32([[10.0, 10.0, 10.0]])])             # outside every box
    return table, rcp, cloud, np.ascontiguousarray(q, np.float32)


def run(mpss, torch, cfg):
    table, rcp, cloud, q = case()
    cfg = dict(cfg)
    if cfg.pop("rgb", False):  # an rgbprofile LayeredSkin: three lookups per record, FromRGB per group
        ctx = mpss.Context(max_error=MAX_ERROR, exact_mo=0, **cfg)
        mid = ctx.add_layeredskin(mpss.default_skin(rgb_profile=1, desired_length=512, **RGB_SKIN))
        cloud = (cloud[0] * np.float32(RGB_SCALE),) + tuple(cloud[1:])
        q = np.ascontiguousarray(q * np.float32(RGB_SCALE))
    else:
        ctx = mpss.Context(max_error=MAX_ERROR, exact_mo=0, **cfg)
        mid = ctx.set_material_tables(table, rcp, np.zeros(1025, np.float32))
    ctx.set_irradiance_points(*cloud)
    qd = torch.from_numpy(q).cuda()
    out = torch.zeros((len(q), 30), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((len(q), 4), dtype=torch.int32, device="cuda")
    ctx.mo_batch(mid, len(q), qd.data_ptr(), out.data_ptr())
    ctx.mo_batch(mid, len(q), qd.data_ptr(), torch.zeros_like(out).data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    grid = ctx.gather_info(mid)["common_grid"]
    ctx.close()
    return out.cpu().numpy(), cnt.cpu().numpy(), grid


def paths(mpss, torch, cfg):
    """The instrumented pass's statistics of the case, summed over the band groups."""
    table, rcp, cloud, q = case()
    ctx = mpss.Context(max_error=MAX_ERROR, exact_mo=0, **cfg)
    mid = ctx.set_material_tables(table, rcp, np.zeros(1025, np.float32))
    ctx.set_irradiance_points(*cloud)
    qd = torch.from_numpy(q).cuda()
    out = torch.zeros((len(q), 30), dtype=torch.float32, device="cuda")
    stats = ctx.mo_batch_paths(mid, len(q), qd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    return out.cpu().numpy(), stats


def record(mpss, torch):
    """The golden file's arrays (run against the build to pin)."""
    out = {}
    for name, cfg in VARIANTS.items():
        o, c, g = run(mpss, torch, cfg)
        out["out_" + name], out["cnt_" + name], out["grid_" + name] = o, c, np.bool_(g)
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_case_reaches_the_paths(golden):
    table, rcp, cloud, q = case()
    assert len(q) == 200 and len(q) % 64 == 8
    d2 = ((q[:, None, :].astype(np.float64) - cloud[0][None, :, :]) ** 2).sum(-1)
    for nf in (5088, 10236):
        s_lo, s_hi = d2 * rcp.min(), d2 * rcp.max()
        assert (s_hi < nf).any()                        # every band inside the near field: the LDS path
        for s in (s_lo, s_hi):                          # the widest and the narrowest band past the near
            assert ((s >= nf) & (s < L - 1)).any()      # field, inside the profile: rows / own tables
        assert ((s_lo < L - 1) & (s_hi >= L - 1)).any()  # past some bands' end only: the zero pair
        assert (s_lo >= L - 1).any()                    # past every band's end: zero terms, pruned subtrees
    assert golden["grid_cg_5088"] and golden["grid_cg_10236"] and not golden["grid_bands_5088"]
    assert golden["grid_rgb_cg_5088"] and (golden["out_rgb_cg_5088"][:196] > 0).any()
    cnt = golden["cnt_cg_5088"]
    # nodes and points visited, summed over the 8 groups; the far query is pruned at the root by every group
    assert (cnt[:199, 2] > 8).all()
    lit = q[:198, 0] < 0.6 * RADII[0]                   # away from the black cap, whose leaves hold no live point
    assert lit.sum() > 100 and (cnt[:198, 3][lit] > 0).all()
    assert cnt[199, 2] == 8 and cnt[199, 3] == 0
    live = (cloud[2].reshape(len(cloud[0]), -1).max(axis=1) > 0).sum()
    assert 0 < live < len(cloud[0])                     # black points: leaves with odd live counts, black nodes


# the statistics' slots (include/mpss.h, mpss_mo_batch_paths)
PATH_SLOTS = {"node visits": 0, "point visits": 1, "group rows": 8, "LDS near field": 9, "own tables": 10,
              "flagged row cell": 17, "near leaf (LDS pair loop)": 18, "odd live count": 19,
              "pruned subtree": 20, "black node": 21, "inside a node's box": 22}


@pytest.mark.parametrize("name", ["cg_5088", "cg_10236"])
def test_walk_takes_every_path(mpss, golden, name):
    """The instrumented pass over the same case: every path of the walk and of the lookup occurs at least
    once (its lane-record and path counters, summed over the band groups), every band group walks, and
    the pass returns the pinned sums."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    out, stats = paths(mpss, torch, VARIANTS[name])
    assert stats.shape == (8, 23)
    total = stats.sum(axis=0)
    for what, slot in PATH_SLOTS.items():
        print(name, what, int(total[slot]))
    for what, slot in PATH_SLOTS.items():
        assert total[slot] > 0, what
    assert (stats[:, 0] > 0).all() and (stats[:, 1] > 0).all()      # all 8 band groups are non-empty
    cnt = golden["cnt_" + name]
    assert int(total[0]) == int(cnt[:, 2].sum()) and int(total[1]) == int(cnt[:, 3].sum())
    assert np.array_equal(out.view(np.uint32), golden["out_" + name].view(np.uint32))


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_node_loop_bit_identical(mpss, golden, name):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    out, cnt, grid = run(mpss, torch, VARIANTS[name])
    assert bool(grid) == bool(golden["grid_" + name])
    assert np.array_equal(cnt, golden["cnt_" + name])
    want = golden["out_" + name]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), np.abs(out - want).max()
