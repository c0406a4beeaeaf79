"""The host grid builder under sanitizers, on the CPU: tests/cg_host/cg_host.cpp links
csrc/common_grid.cpp alone (plain C++: no libmpss, no HIP runtime, no GPU), both compiled with the ROCm
clang and -fsanitize=address,undefined -fno-sanitize-recover=all. It builds the grids of three pinned
cases (tests/test_common_grid_pinned.py: the rough table, the one whose rows go H > 1 steps apart, the
rgbprofile) for both LDS layouts in a child process, which must exit 0 with nothing reported.
"""
import os
import subprocess

import numpy as np

from test_common_grid_pinned import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrt-v2-skin_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")


def test_grid_builder_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "cg_host")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cg_host", "cg_host.cpp"), os.path.join(CSRC, "common_grid.cpp"),
                    "-lpthread", "-o", exe], check=True)
    files = []
    for name in ("rough", "coarse", "rgb"):
        tab, rcp, kw = _case(name)
        mode = 2 if kw.get("rgb") else int(bool(kw.get("snake")))
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(np.array([tab.shape[1], mode], np.int32).tobytes())
            f.write(np.ascontiguousarray(rcp, np.float32).tobytes())
            f.write(np.ascontiguousarray(tab, np.float32).tobytes())
        files.append(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr.strip() == "", r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 6 and all(" ok 1 " in ln for ln in lines), r.stdout
    # the cases still reach their branches: flagged cells in the rough table, coarse rows in the long one
    assert all(" flagged 0 " not in ln for ln in lines[:2]), r.stdout
    assert all(float(ln.split()[-1]) < 1.0 for ln in lines[2:4]), r.stdout
