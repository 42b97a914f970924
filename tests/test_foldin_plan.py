"""csrc/foldin_plan.h: the host-only cut of an implicit fold-in request into dual rows, primal units and empty rows.
tests/cpp/foldin_plan_test.cc is a stand-alone program over that header alone, built with g++ and the host sanitizers and run as
a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "you-can-not-recommend_amd", "csrc")


def test_foldin_plan_header_on_the_cpu_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "foldin_plan_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "foldin_plan_test.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "foldin_plan_test: ok" in r.stdout
