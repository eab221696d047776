"""The C++ host mirror's wall deviation map (host/gm_surface_test.cpp, plain g++ over the C ABI): Processor::
setSurfaceParams and Processor::getSurfaceMap."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_surface_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_surface_test"], check=True, capture_output=True)


def test_host_surface_map_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "void setSurfaceParams(const gm_surface_params &params);" in hdr
    assert "void getSurfaceMap(gm_surface_info &info, std::vector<gm_surface_cell> &cells);" in hdr


@pytest.mark.gpu
def test_host_surface_map_on_gpu():
    _build()
    r = subprocess.run([EXE, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_surface_test ok" in r.stdout
