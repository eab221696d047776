"""The C++ host mirror's wall map on a clothoid design axis (host/gm_wall_clothoid_test.cpp, plain g++ over the C ABI):
Processor::createWallMap(params, NULL, clothoid), then a drive of three frames (check, add) and one cloud against the C
ABI's bytes, and the refusals of locateWallMap and alignWallMap."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_clothoid_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_clothoid_test"], check=True, capture_output=True)


def test_host_wall_clothoid_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "void createWallMap(const gm_wall_params &params, const gm_wall_arc *arc, const gm_wall_clothoid *clothoid);" in hdr
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    lines = mk.splitlines()
    for head in ("all:", "gm_wall_clothoid_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_clothoid_test") for ln in lines if ln.startswith(head)] == [1], head
    assert sum("gm_wall_clothoid_test.cpp" in ln and ln.startswith("\t$(CXX)") for ln in lines) == 1   # the rule's command


@pytest.mark.gpu
def test_host_wall_clothoid_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_clothoid_test ok" in r.stdout
