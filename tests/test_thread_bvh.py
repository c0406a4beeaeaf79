"""thread_bvh (csrc/scene_plain.cpp) on the CPU: the threaded BVH copy that upload_scene puts on the device for the
stackless any-hit tracers of bvh_trace.h. tests/thread_bvh_host/thread_bvh_host.cpp links the unit alone (plain C++: no
libmpss, no HIP runtime, no GPU), both compiled with the ROCm clang and -fsanitize=address,undefined
-fno-sanitize-recover=all. One child process threads every tree -- the pinned ones of tests/golden/thread_bvh_pins.json
(their offsets as the loop inside upload_scene gave them before it became a function) and random pre-order skeletons --
and must exit 0 with nothing reported; the properties the tracers rely on are checked here.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrt-v2-skin_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")

with open(os.path.join(ROOT, "tests", "golden", "thread_bvh_pins.json")) as _f:
    PINS = json.load(_f)["trees"]


def skeleton(n_leaves, rng, lean=None):
    """A binary tree of n_leaves leaves in pre-order, as [nprims, offset] per node: a leaf has nprims > 0 and offset =
    its first primitive, an interior node nprims 0 and offset = its second child (the first is the next node).
    lean: None splits at random, 0 / 1 always puts one leaf left / right (a chain)."""
    nodes, prim = [], [0]

    def build(k):  # (the recursion is as deep as the tree: at most 150 here)
        i = len(nodes)
        if k == 1:
            nodes.append([int(rng.integers(1, 5)), prim[0]])
            prim[0] += nodes[-1][0]
            return
        nodes.append([0, -1])
        left = 1 if lean == 0 else k - 1 if lean == 1 else int(rng.integers(1, k))
        build(left)
        nodes[i][1] = len(nodes)
        build(k - left)

    build(n_leaves)
    return nodes


def _trees():
    rng = np.random.default_rng(20240918)
    trees = [skeleton(1, rng), skeleton(2, rng), skeleton(150, rng, lean=0), skeleton(150, rng, lean=1)]
    trees += [skeleton(int(rng.integers(2, 200)), rng) for _ in range(200)]
    return trees


@pytest.fixture(scope="module")
def threaded(tmp_path_factory):
    """(tree, threaded offsets) of every pinned and generated tree, from ONE run of the sanitized host program."""
    tmp = tmp_path_factory.mktemp("thread_bvh")
    exe = str(tmp / "thread_bvh_host")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + CSRC, os.path.join(ROOT, "tests", "thread_bvh_host", "thread_bvh_host.cpp"),
                    os.path.join(CSRC, "scene_plain.cpp"), "-o", exe], check=True)
    trees = [p["nodes"] for p in PINS] + _trees()
    path = str(tmp / "trees.txt")
    with open(path, "w") as f:
        for t in trees:
            f.write("%d %s\n" % (len(t), " ".join("%d %d" % (a, b) for a, b in t)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stderr.strip() == "", r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(trees)
    return list(zip(trees, out))


def _subtree_end(t, i):
    return i + 1 if t[i][0] > 0 else _subtree_end(t, t[i][1])


def _walk(t, off, hit):
    """The stackless walk of bvh_trace.h over the threaded offsets: from a node whose box is hit on to i + 1 (an
    interior node's first child, or what follows a leaf), from a missed one to the end of its subtree."""
    i, seen = 0, []
    while i < len(t):
        seen.append(i)
        i = i + 1 if hit[i] or t[i][0] > 0 else off[i]
    assert i == len(t)  # it ends at size exactly
    return seen


def _with_stack(t, hit):
    """The same traversal with a stack over the plain offsets: the nodes all of whose ancestors were hit, in pre-order."""
    seen, stack = [], [0]
    while stack:
        i = stack.pop()
        seen.append(i)
        if t[i][0] == 0 and hit[i]:
            stack += [t[i][1], i + 1]
    return seen


def test_thread_pins(threaded):
    for p, (t, off) in zip(PINS, threaded):
        assert t == p["nodes"] and off == p["threaded"]


def test_threaded_offsets(threaded):
    rng = np.random.default_rng(5)
    trees = threaded[len(PINS):]
    assert len(trees[0][0]) == 1  # the single leaf
    for k, lean in ((2, 0), (3, 1)):  # the two chains: every interior node has a leaf on one side
        t = trees[k][0]
        assert len(t) == 299 and all(t[i + 1 if lean == 0 else t[i][1]][0] > 0 for i in range(len(t)) if t[i][0] == 0)
    for t, off in trees:
        n = len(t)
        assert len(off) == n
        for i, (nprims, offset) in enumerate(t):
            if nprims > 0:
                assert off[i] == offset  # leaves are untouched
            else:
                assert off[i] == _subtree_end(t, i)  # an interior node: the end of its pre-order subtree
        # the rule i = leaf ? i + 1 : offset of a walk that misses everything: on the plain offsets it runs down the
        # root's right spine to the last node, on the threaded ones it leaves the root's subtree at once; both end at n
        i, spine = 0, []
        while i < n:
            spine.append(i)
            i = i + 1 if t[i][0] > 0 else t[i][1]
        assert i == n and spine[-1] == n - 1 and all(t[a][1] == b for a, b in zip(spine, spine[1:]))
        assert _walk(t, off, [False] * n) == [0]
        # every subtree a walk skips ends where a node of that spine's kind begins: at n or at a second child
        seconds = {n} | {t[i][1] for i in range(n) if t[i][0] == 0}
        assert all(off[i] in seconds for i in range(n) if t[i][0] == 0)
        # a walk that hits everything visits each node once, in pre-order; one that hits some, what a stack would
        assert _walk(t, off, [True] * n) == list(range(n))
        for _ in range(4):
            hit = list(rng.random(n) < 0.7)
            assert _walk(t, off, hit) == _with_stack(t, hit)
