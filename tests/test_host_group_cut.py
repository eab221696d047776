"""The slab cut of a group (csrc/gm_group_cut.hpp: the histogram over the voxel lattice, the edges, the per-thread counts
and the scatter) on the CPU, under AddressSanitizer + UBSan and under ThreadSanitizer.

host/gm_group_cut_test.cpp is a stand-alone program that includes that header and nothing else of the library: it
initialises no device and calls no HIP function.  The cut takes its thread count as an argument, so the threaded passes
run here at a few thousand rows.  Nothing loaded into Python is sanitised."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "geometric_mapping_amd", "csrc", "gm_group_cut.hpp")


def test_the_cut_header_is_device_free():
    src = open(HEADER).read()
    assert re.search(r"\bhip[A-Z]\w*\s*\(", src) is None   # the file calls no HIP function
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert "../../include/gm_hip.h" in includes
    assert not [i for i in includes if "hip/" in i or i.startswith("gm_")], includes


@pytest.mark.parametrize("san", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["-fsanitize=thread"]],
                         ids=["asan_ubsan", "tsan"])
def test_the_cut_runs_cleanly_under_sanitizers(tmp_path, san):
    exe = str(tmp_path / "gm_group_cut_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror"] + san +
                   [os.path.join(ROOT, "host", "gm_group_cut_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gm_group_cut_test ok"), r.stdout + r.stderr
