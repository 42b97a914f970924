"""csrc/schedule.h: the host-only work-unit scheduler (how an upload is cut into units, in which order a split row's partial
sums are added).  tests/cpp/schedule_test.cc is a stand-alone program over that header alone: it is built with g++ and the
host sanitizers (their runtimes linked into the program) and run as a child process; the properties and literal cases it
checks are listed in its test functions."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "you-can-not-recommend_amd", "csrc")


def test_schedule_header_on_the_cpu_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "schedule_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "schedule_test.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "schedule_test: ok" in r.stdout


def test_schedule_header_is_host_only():
    """No HIP include, no environment, no device call: the header must stay compilable by a plain C++ compiler."""
    text = open(os.path.join(CSRC, "schedule.h")).read()
    for word in ("hip/", "getenv", "hipMalloc", "hipMemcpy", "__global__", "__device__"):
        assert word not in text, word
