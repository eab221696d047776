"""The C++ host mirror's align on a wall alignment (host/gm_wall_alignment_align_test.cpp, plain g++ over the C ABI):
Processor::alignWallAlignment across the clothoid -> arc joint must give the C ABI's info and score table, byte for byte,
and the shift the frame's pose was given."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_alignment_align_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_alignment_align_test"], check=True, capture_output=True)


def test_host_wall_alignment_align_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "gm_wall_alignment_align_info alignWallAlignment(const double pose[12], const gm_wall_align_params &prm," in hdr
    lines = open(os.path.join(ROOT, "host", "Makefile")).read().splitlines()
    for head in ("all:", "gm_wall_alignment_align_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_alignment_align_test") for ln in lines if ln.startswith(head)] == [1], head


@pytest.mark.gpu
def test_host_wall_alignment_align_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_alignment_align_test ok" in r.stdout


def test_align_host_entries_run_cleanly_under_sanitizers(tmp_path):
    """The device-free half (gm_wall_alignment_align_plan, _align_select) as a stand-alone program under AddressSanitizer
    and UBSan (host/gm_wall_alignment_align_host_test.cpp, linked with gm_wall_host.hip and gm_wall_alignment_host.hip alone:
    no device, no Python)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "gm_wall_alignment_align_host_test")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    csrc = os.path.join(ROOT, "geometric_mapping_amd", "csrc")
    subprocess.run([os.path.join(rocm, "bin", "hipcc"), "--offload-host-only", "-std=c++17", "-O1", "-g"] + san +
                   [os.path.join(csrc, "gm_wall_host.hip"), os.path.join(csrc, "gm_wall_alignment_host.hip"),
                    os.path.join(ROOT, "host", "gm_wall_alignment_align_host_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gm_wall_alignment_align_host_test ok"), r.stdout + r.stderr
