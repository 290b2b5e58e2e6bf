"""The guard every extern "C" entry of libzkg.so goes through (zklaim_amd/csrc/c_boundary.hpp), as a stand-alone C++ program built with the
address and undefined-behaviour sanitizers: no GPU, no HIP headers, set_error stubbed."""
import os
import subprocess


def test_c_boundary_guard(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_boundary_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tests", "c", "c_boundary_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0 and "c_boundary ok" in out.stdout
