"""The C++ host mirror's check and checked add on a wall alignment (host/gm_wall_alignment_check_test.cpp, plain g++ over
the C ABI): Processor::checkWallAlignment and addToWallAlignmentChecked across the clothoid -> arc joint must give the C
ABI's info, rows and element maps, byte for byte."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_alignment_check_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_alignment_check_test"], check=True, capture_output=True)


def test_host_wall_alignment_check_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "std::vector<gm_wall_check_point> checkWallAlignment(const double pose[12], const gm_wall_check_params &prm," in hdr
    assert "gm_wall_alignment_add_info addToWallAlignmentChecked(const double pose[12], const gm_wall_add_checked_params &prm," in hdr
    lines = open(os.path.join(ROOT, "host", "Makefile")).read().splitlines()
    for head in ("all:", "gm_wall_alignment_check_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_alignment_check_test") for ln in lines if ln.startswith(head)] == [1], head


@pytest.mark.gpu
def test_host_wall_alignment_check_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_alignment_check_test ok" in r.stdout
