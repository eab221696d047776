"""The C++ host mirror's cylinder regression (host/gm_cylfit_test.cpp, plain g++ over the C ABI): Processor::getCylinder
and the rvizCylinder overload that takes a gm_cylinder_fit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_cylfit_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_cylfit_test"], check=True, capture_output=True)


def test_host_cylinder_fit_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "gm_cylinder_fit getCylinder(" in hdr and "rvizCylinder(const gm_cylinder_fit &fit" in hdr


@pytest.mark.gpu
def test_host_get_cylinder_and_marker_on_gpu():
    _build()
    r = subprocess.run([EXE, "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_cylfit_test ok" in r.stdout
