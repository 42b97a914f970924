"""csrc/owned.h: the host-only move-only owner (Owned) and grow-only buffer (GrowBuf) that hold every device buffer, pinned
host buffer, event and stream of ycnr_als.hip.  tests/cpp/owned_test.cc is a stand-alone program over that header alone, with
counting free / allocate policies: it is built with g++ and the host sanitizers (their runtimes linked into the program) and
run as a child process; the properties it checks are listed in its test functions."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "you-can-not-recommend_amd", "csrc")


def test_owned_header_on_the_cpu_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "owned_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "owned_test.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "owned_test: ok" in r.stdout


def test_owned_header_is_host_only():
    """No HIP include, no environment, no device call: the header must stay compilable by a plain C++ compiler (the free and
    allocate calls are policies that ycnr_als.hip supplies)."""
    text = open(os.path.join(CSRC, "owned.h")).read()
    for word in ("hip/", "getenv", "hipMalloc", "hipFree", "__global__", "__device__"):
        assert word not in text, word
