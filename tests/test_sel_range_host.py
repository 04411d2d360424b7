"""SelRange (the fused selection's range test, csrc/sel_pred.hpp) equals sel_one (the unfused int64
compare) for every int64 constant: tests/cpp/sel_range_host.cc, a stand-alone host program, built with
the host compiler under UndefinedBehaviorSanitizer (a signed overflow in SelRange::from aborts it) and
run. No GPU, nothing loaded into Python.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sel_range_equals_sel_one_host(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "sel_range_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "3d-hashjoin_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "sel_range_host.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
