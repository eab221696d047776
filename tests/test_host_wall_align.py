"""The C++ host mirror's wall-map align (host/gm_wall_align_test.cpp, plain g++ over the C ABI): Processor::alignWallMap
against a direct gm_wall_map_align_frame / gm_wall_map_get_align call, the stage call, the host-only selection on the
returned table and the true pose of a synthetic frame on a textured wall."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_align_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_align_test"], check=True, capture_output=True)


def test_host_wall_align_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "gm_wall_align_info alignWallMap(const double pose[12], const gm_wall_align_params &prm," in hdr
    assert "std::vector<gm_wall_align_score> *scores = nullptr);" in hdr
    assert "locateWallMap,\n    // alignWallMap with the located pose, then checkWallMap and addToWallMap with the aligned pose." in hdr
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    lines = mk.splitlines()
    for head in ("all:", "gm_wall_align_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_align_test") for ln in lines if ln.startswith(head)] == [1], head
    assert sum("gm_wall_align_test.cpp" in ln and ln.startswith("\t$(CXX)") for ln in lines) == 1   # the rule's command
    assert "host/gm_wall_align_test" in open(os.path.join(ROOT, ".gitignore")).read().split()


@pytest.mark.gpu
def test_host_wall_align_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_align_test ok" in r.stdout
