"""csrc/step_policy.h: the host-only rules that say which of the three paths a solve takes (one wave per row, a workgroup per
row, any k), the parameters of a piece's plan, the predicates every half-step consults, whether the dual classes go to side
streams, and the launch geometry of the any-k path.  tests/cpp/step_policy_test.cc is a stand-alone program over that header
alone: it is built with g++ and the host sanitizers (their runtimes linked into the program) and run as a child process; it
states the rules over every k up to 4096 in both precisions, every (dtype, k <= 256, flags, toggles) with fixed matrices on
each side of the 2 GB and 64 MB limits, and a literal case per quirk."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "you-can-not-recommend_amd", "csrc")


def test_step_policy_header_on_the_cpu_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "step_policy_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "step_policy_test.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "step_policy_test: ok (8192 paths, 262144 shapes, 63488 any-k launches)" in r.stdout


def test_step_policy_header_is_host_only():
    """No HIP include, no environment, no device call: the header must stay compilable by a plain C++ compiler.  The one
    host/device marker (YCNR_HD, for the sizing functions the kernels share) is the only place that names the device."""
    text = open(os.path.join(CSRC, "step_policy.h")).read()
    for word in ("hip/", "hip_runtime", "getenv", "hipMalloc", "hipMemcpy", "hipLaunch", "hipStream", "hipEvent", "hipFunc", "__global__", "__shared__"):
        assert word not in text, word
    assert re.findall(r".*__device__.*", text) == ["#define YCNR_HD __host__ __device__"]
    assert re.findall(r"#include\s+(\S+)", text) == ['"../../include/ycnr_als.h"', '"schedule.h"']
