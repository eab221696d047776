"""The C++ host mirror's wall alignment (host/gm_wall_alignment_test.cpp, plain g++ over the C ABI):
Processor::createWallAlignment and addToWallAlignment on frames across two joints against the C ABI's bytes; and the
device-free calls as a stand-alone program under AddressSanitizer and UBSan (host/gm_wall_alignment_host_test.cpp, linked
with gm_wall_host.hip and gm_wall_alignment_host.hip alone: no device, no Python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
EXE = os.path.join(ROOT, "host", "gm_wall_alignment_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_alignment_test"], check=True, capture_output=True)


def test_host_wall_alignment_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "void createWallAlignment(const gm_wall_params &params, const std::vector<gm_wall_element> &elements);" in hdr
    assert "gm_wall_alignment_add_info addToWallAlignment(const double pose[12]);" in hdr
    assert "gm_wall_alignment *wallAlignment()" in hdr
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    lines = mk.splitlines()
    for head in ("all:", "gm_wall_alignment_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_alignment_test") for ln in lines if ln.startswith(head)] == [1], head
    assert sum("gm_wall_alignment_test.cpp" in ln and ln.startswith("\t$(CXX)") for ln in lines) == 1   # the rule's command


def test_alignment_host_entries_run_cleanly_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gm_wall_alignment_host_test")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    csrc = os.path.join(ROOT, "geometric_mapping_amd", "csrc")
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "--offload-host-only", "-std=c++17", "-O1", "-g"] + san +
                   [os.path.join(csrc, "gm_wall_host.hip"), os.path.join(csrc, "gm_wall_alignment_host.hip"),
                    os.path.join(ROOT, "host", "gm_wall_alignment_host_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gm_wall_alignment_host_test ok"), r.stdout + r.stderr


@pytest.mark.gpu
def test_host_wall_alignment_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_alignment_test ok" in r.stdout
