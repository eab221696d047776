"""The C++ host mirror's objects of a check (host/gm_wall_objects_test.cpp, plain g++ over the C ABI):
Processor::wallCheckObjects against a direct gm_wall_map_check_objects call, the stage call gm_wall_check_objects and a
scalar C++ restatement of the rule (a flood fill) on an 80 x 90 map."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_objects_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_objects_test"], check=True, capture_output=True)


def test_host_wall_objects_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert ("std::vector<gm_wall_object> wallCheckObjects(const gm_wall_object_params &prm, "
            "gm_wall_objects_info *info = nullptr);") in hdr
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    lines = mk.splitlines()
    for head in ("all:", "gm_wall_objects_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_objects_test") for ln in lines if ln.startswith(head)] == [1], head
    assert sum("gm_wall_objects_test.cpp" in ln and ln.startswith("\t$(CXX)") for ln in lines) == 1   # the rule's command


@pytest.mark.gpu
def test_host_wall_objects_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_objects_test ok" in r.stdout
