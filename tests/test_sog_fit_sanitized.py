"""The host fit unit under sanitizers, on the CPU: tests/sog_host/sog_host.cpp links csrc/profile_fit.cpp alone
(plain C++: no libmpss, no HIP runtime, no GPU), both compiled with the ROCm clang and
-fsanitize=address,undefined -fno-sanitize-recover=all. The program runs the host fit on fixed inputs (1, 2, 87
and 1162 samples; a profile without a candidate among them) in a child process, which must exit 0 with nothing
reported.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrt-v2-skin_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")


def test_host_fit_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sog_host")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "sog_host", "sog_host.cpp"), os.path.join(CSRC, "profile_fit.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr.strip() == "", r.stderr
    assert r.stdout.strip().endswith("all ok 0"), r.stdout
