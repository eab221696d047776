"""The C++ host mirror's persistent wall map (host/gm_wall_test.cpp, plain g++ over the C ABI): Processor::createWallMap,
addToWallMap, readWallMap and wallMapInfo."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_test"], check=True, capture_output=True)


def test_host_wall_map_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "void createWallMap(const gm_wall_params &params);" in hdr
    assert "gm_wall_add_info addToWallMap(const double pose[12]);" in hdr
    assert "void readWallMap(unsigned station0, unsigned n, std::vector<gm_surface_cell> &cells);" in hdr


@pytest.mark.gpu
def test_host_wall_map_on_gpu():
    _build()
    r = subprocess.run([EXE, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_test ok" in r.stdout
