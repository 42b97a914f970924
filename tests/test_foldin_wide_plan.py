"""csrc/foldin_wide_plan.h: the host-only cut of a request of ycnr_als_fold_in_implicit_wide into short served, long served,
unserved and empty rows, and the LDS sizes its kernel shares with the launch code.  tests/cpp/foldin_wide_plan_test.cc is a
stand-alone program over that header alone, built with g++ and the host sanitizers and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "you-can-not-recommend_amd", "csrc")


def test_foldin_wide_plan_header_on_the_cpu_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "foldin_wide_plan_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "foldin_wide_plan_test.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "foldin_wide_plan_test: ok" in r.stdout
