"""The MSM's host epilogue (zklaim_amd/csrc/host/horner_jac.hpp: the dedicated squaring, runs of Jacobian doublings, Horner over the windows)
against the general product and the XYZZ doublings it replaces, as a stand-alone program (tools/host_epilogue_check.hip, host code only: no
GPU is touched) built with the address and undefined-behaviour sanitizers."""
import os
import subprocess


def test_host_epilogue_old_against_new(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_epilogue_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tools", "host_epilogue_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0 and "ok: squares, runs of doublings and Horner agree" in out.stdout
