"""The C++ host mirror's check objects on a wall alignment (host/gm_wall_alignment_objects_test.cpp, plain g++ over the C
ABI): Processor::wallAlignmentCheckObjects across the clothoid -> arc joint must give one object through the joint plane and
the C ABI's info and records, byte for byte."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_alignment_objects_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_alignment_objects_test"], check=True, capture_output=True)


def test_host_wall_alignment_objects_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert ("std::vector<gm_wall_object> wallAlignmentCheckObjects(const gm_wall_object_params &prm, "
            "gm_wall_alignment_objects_info *info = nullptr);") in hdr
    lines = open(os.path.join(ROOT, "host", "Makefile")).read().splitlines()
    for head in ("all:", "gm_wall_alignment_objects_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_alignment_objects_test") for ln in lines if ln.startswith(head)] == [1], head


@pytest.mark.gpu
def test_host_wall_alignment_objects_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_alignment_objects_test ok" in r.stdout
