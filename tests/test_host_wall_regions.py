"""The C++ host mirror's deviation regions (host/gm_wall_regions_test.cpp, plain g++ over the C ABI):
Processor::wallMapRegions on a short drive with three world-fixed patches."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_regions_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_regions_test"], check=True, capture_output=True)


def test_host_wall_regions_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert ("std::vector<gm_wall_region> wallMapRegions(unsigned station0, unsigned n, const gm_wall_region_params &prm, "
            "gm_wall_regions_info *info = nullptr);") in hdr
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    assert mk.count("gm_wall_regions_test") >= 4   # all, the rule, its command, clean


@pytest.mark.gpu
def test_host_wall_regions_on_gpu():
    _build()
    r = subprocess.run([EXE, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_regions_test ok" in r.stdout
