"""The C++ host mirror's checked add (host/gm_wall_add_checked_test.cpp, plain g++ over the C ABI):
Processor::addToWallMapChecked against gm_wall_map_add_points of the cloud less the rows a scalar C++ restatement of the rule
selects, and against the stage call gm_wall_map_add_points_checked, on an 80 x 90 map."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_add_checked_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_add_checked_test"], check=True, capture_output=True)


def test_host_wall_add_checked_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert ("gm_wall_add_info addToWallMapChecked(const double pose[12], const gm_wall_add_checked_params &prm, "
            "gm_wall_add_checked_info *info = nullptr);") in hdr
    assert "checkWallMap, addToWallMapChecked" in hdr   # the ordering comment
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    lines = mk.splitlines()
    for head in ("all:", "gm_wall_add_checked_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_add_checked_test") for ln in lines if ln.startswith(head)] == [1], head
    assert sum("gm_wall_add_checked_test.cpp" in ln and ln.startswith("\t$(CXX)") for ln in lines) == 1   # the rule's command
    assert "host/gm_wall_add_checked_test" in open(os.path.join(ROOT, ".gitignore")).read().split()


@pytest.mark.gpu
def test_host_wall_add_checked_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_add_checked_test ok" in r.stdout
