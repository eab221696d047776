"""The memory owners (csrc/gm_dev_array.hpp: DevArray, HostArray) on the CPU, under AddressSanitizer and UBSan.

host/gm_dev_array_test.cpp is a stand-alone program: it defines the four HIP allocation calls itself on top of malloc and
free, so it needs no device and no HIP runtime, only the HIP headers.  Nothing loaded into Python is sanitised."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_owners_grow_fail_move_and_release_cleanly_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gm_dev_array_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                    os.path.join(ROOT, "host", "gm_dev_array_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_dev_array_test ok" in r.stdout
