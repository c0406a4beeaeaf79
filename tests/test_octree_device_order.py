"""device_order (csrc/octree.cpp) on the CPU: the leaf reorder DeviceOctree::upload applies before it copies the host
tree to the device -- each leaf's black points (E == 0) behind its other points, and the count of the others in
NodeHdr::pad -- which the sharded gather's leaf loop relies on (mo_band.h) and tests/test_octree_gpu.py checks on the GPU.
tests/octree_order_host/octree_order_host.cpp links octree.cpp alone (host C++: no libmpss, no GPU), both compiled with
the ROCm clang and -fsanitize=address,undefined -fno-sanitize-recover=all. One child process builds every cloud with
build_octree and prints the host tree beside device_order's copy; it must exit 0 with nothing reported, and the copy is
compared with the rule restated in numpy.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrt-v2-skin_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CLANG = os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
ROW = 32
# NodeHdr's words (octree.h): skip, leaf_first, leaf_count, depth, flags, pad
W_LEAF_FIRST, W_LEAF_COUNT, W_PAD = 11, 12, 15

# the black points of the eight full leaves of the "slots" cloud, by leaf slot (bit s: the leaf's s-th point): the
# first only, the last only, the two interleavings, the first half, the last half, all, none
SLOT_MASKS = (0x01, 0x80, 0x55, 0xaa, 0x0f, 0xf0, 0xff, 0x00)


def _clouds():
    """name -> (P n x 3, area n, black n)"""
    rng = np.random.default_rng(20241020)
    n = 300
    P = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    area = rng.uniform(0.5, 2.0, n).astype(np.float32)
    clouds = {"no_black": (P, area, np.zeros(n, bool))}
    # every point left of x = -0.3 is black (whole leaves), 30 % of the others
    clouds["black_leaves"] = (P, area, (P[:, 0] < -0.3) | (rng.random(n) < 0.3))
    # eight clusters of eight points at the corners of a cube: the root splits into eight full leaves; point i
    # belongs to cluster i % 8 and is its (i // 8)-th point
    corner = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    i = np.arange(64)
    Ps = (corner[i % 8] + rng.uniform(-0.01, 0.01, (64, 3))).astype(np.float32)
    clouds["slots"] = (Ps, np.ones(64, np.float32), np.array([(SLOT_MASKS[k % 8] >> (k // 8)) & 1 for k in i], bool))
    clouds["single_leaf"] = (P[:5], area[:5], np.array([1, 0, 1, 0, 0], bool))
    return clouds


CLOUDS = _clouds()


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """name -> {"flat": ..., "dev": ...} as uint32 arrays, from ONE run of the sanitized host program."""
    tmp = tmp_path_factory.mktemp("octree_order")
    exe = str(tmp / "octree_order_host")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC, "-I" + os.path.join(ROCM, "include"),
                    os.path.join(ROOT, "tests", "octree_order_host", "octree_order_host.cpp"),
                    os.path.join(CSRC, "octree.cpp"), "-o", exe], check=True)
    path = str(tmp / "clouds.txt")
    with open(path, "w") as f:
        for P, area, black in CLOUDS.values():
            f.write("%d\n" % len(P))
            for p, a, b in zip(P, area, black):
                f.write("%.9g %.9g %.9g %.9g %d\n" % (p[0], p[1], p[2], a, b))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stderr.strip() == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(CLOUDS)
    out = {}
    for name, line in zip(CLOUDS, lines):
        d = json.loads(line)
        out[name] = {k: {"hdr": np.array(v["hdr"], np.uint32).reshape(-1, 16),
                         "pt_hdr": np.array(v["pt_hdr"], np.uint32).reshape(-1, 4),
                         "pt_e": np.array(v["pt_e"], np.uint32).reshape(-1, ROW),
                         "pt_index": np.array(v["pt_index"], np.uint32)} for k, v in d.items()}
    return out


def _leaves(hdr):
    """(node, first, count) of every leaf"""
    first = hdr[:, W_LEAF_FIRST].view(np.int32)
    return [(i, int(first[i]), int(hdr[i, W_LEAF_COUNT])) for i in range(len(hdr)) if first[i] >= 0]


def _black(pt_hdr):
    return (pt_hdr[:, 3] >> 31).astype(bool)  # the area's sign bit


def _check(name, t):
    """The rule, leaf by leaf; returns the leaves as (count, black flags in the host tree's order)."""
    flat, dev = t["flat"], t["dev"]
    P, area, black_in = CLOUDS[name]
    n = len(P)
    assert len(flat["pt_index"]) == n and sorted(flat["pt_index"]) == list(range(n))
    black = _black(flat["pt_hdr"])
    assert np.array_equal(black, black_in[flat["pt_index"]])  # the host tree marks the points the cloud made black
    for k in ("hdr", "pt_hdr", "pt_e", "pt_index"):
        assert dev[k].shape == flat[k].shape
    # nothing in a header changes but pad; the host tree leaves pad 0
    assert np.array_equal(dev["hdr"][:, :W_PAD], flat["hdr"][:, :W_PAD]) and not flat["hdr"][:, W_PAD].any()
    leaves = _leaves(flat["hdr"])
    assert sum(c for _, _, c in leaves) == n
    is_leaf = np.zeros(len(flat["hdr"]), bool)
    is_leaf[[i for i, _, _ in leaves]] = True
    assert not dev["hdr"][~is_leaf, W_PAD].any()  # interior nodes: pad = 0
    seen = []
    for node, first, count in leaves:
        assert 1 <= count <= 8
        b = black[first:first + count]
        order = first + np.concatenate([np.flatnonzero(~b), np.flatnonzero(b)])  # live first, each kind in its order
        pad = int(dev["hdr"][node, W_PAD])
        assert pad & 0xffff == int((~b).sum()) and pad >> 16 == 0
        sl = slice(first, first + count)
        # one permutation for the three arrays (pt_index is unique per point, so it names the permutation)
        assert np.array_equal(dev["pt_index"][sl], flat["pt_index"][order])
        assert np.array_equal(dev["pt_hdr"][sl], flat["pt_hdr"][order])
        assert np.array_equal(dev["pt_e"][sl], flat["pt_e"][order])
        db = _black(dev["pt_hdr"])[sl]
        assert not db[:pad & 0xffff].any() and db[pad & 0xffff:].all()
        # a live point carries its own E row (band 0 = 1 + its index), a black one zeros
        e0 = dev["pt_e"][sl, 0].view(np.float32)
        assert np.array_equal(e0, np.where(db, 0.0, 1.0 + dev["pt_index"][sl]).astype(np.float32))
        seen.append((count, tuple(bool(x) for x in b)))
    return seen


def test_no_black_is_identity(trees):
    t = trees["no_black"]
    leaves = _check("no_black", t)
    assert len(leaves) > 8
    for k in ("pt_hdr", "pt_e", "pt_index"):
        assert np.array_equal(t["dev"][k], t["flat"][k])
    assert np.array_equal(t["dev"]["hdr"][:, :W_PAD], t["flat"]["hdr"][:, :W_PAD])
    for node, _, count in _leaves(t["flat"]["hdr"]):
        assert t["dev"]["hdr"][node, W_PAD] == count


def test_leaves_all_black(trees):
    leaves = _check("black_leaves", trees["black_leaves"])
    assert any(all(b) for _, b in leaves) and any(not any(b) for _, b in leaves)
    assert any(any(b) and not all(b) for _, b in leaves)
    t = trees["black_leaves"]
    black = _black(t["flat"]["pt_hdr"])
    all_black = [n for n, f, c in _leaves(t["flat"]["hdr"]) if black[f:f + c].all()]
    assert all_black and not t["dev"]["hdr"][all_black, W_PAD].any()  # no live point: pad 0


def test_every_slot_of_a_full_leaf(trees):
    leaves = _check("slots", trees["slots"])
    # the root and its eight full leaves, one per mask
    assert len(trees["slots"]["flat"]["hdr"]) == 9 and all(c == 8 for c, _ in leaves)
    masks = sorted(sum(1 << s for s in range(8) if b[s]) for _, b in leaves)
    assert masks == sorted(SLOT_MASKS)
    for s in range(8):  # every slot is black in some mixed leaf and live in another
        mixed = [b for _, b in leaves if any(b) and not all(b)]
        assert any(b[s] for b in mixed) and any(not b[s] for b in mixed)


def test_single_leaf(trees):
    t = trees["single_leaf"]
    assert _check("single_leaf", t) == [(5, (True, False, True, False, False))]
    assert len(t["flat"]["hdr"]) == 1
    assert list(t["dev"]["pt_index"]) == [1, 3, 4, 0, 2] and t["dev"]["hdr"][0, W_PAD] == 3
