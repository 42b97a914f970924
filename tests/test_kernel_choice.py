"""csrc/kernel_choice.h: the host-only rules that say which instantiation of the chunk kernel, the fused row kernel, the reduce
and the band reduce a half-step at k <= 128 runs.  tests/cpp/kernel_choice_test.cc is a stand-alone program over that header
alone: it is built with g++ and the host sanitizers (their runtimes linked into the program) and run as a child process; it
states the rules over every (dtype, k, flags, toggles) and a literal case per quirk."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "you-can-not-recommend_amd", "csrc")


def test_kernel_choice_header_on_the_cpu_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "kernel_choice_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "kernel_choice_test.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "kernel_choice_test: ok (65536 inputs)" in r.stdout


def test_kernel_choice_header_is_host_only():
    """No HIP include, no environment, no device call: the header must stay compilable by a plain C++ compiler."""
    text = open(os.path.join(CSRC, "kernel_choice.h")).read()
    for word in ("hip/", "getenv", "hipMalloc", "hipMemcpy", "__global__", "__device__"):
        assert word not in text, word
