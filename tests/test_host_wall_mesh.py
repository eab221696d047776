"""The C++ host mirror's wall mesh (host/gm_wall_mesh_test.cpp, plain g++ over the C ABI): Processor::wallMapMesh against
a direct gm_wall_map_mesh call, gm_wall_mesh_triangulate and a scalar C++ restatement of the rule on a 65 x 65 map with
holes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_mesh_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_mesh_test"], check=True, capture_output=True)


def test_host_wall_mesh_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert ("void wallMapMesh(unsigned station0, unsigned n, const gm_wall_mesh_params &prm, std::vector<gm_wall_cloud_point> *vertices, "
            "std::vector<gm_wall_mesh_triangle> *triangles, gm_wall_mesh_info *info = nullptr);") in hdr
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    lines = mk.splitlines()
    for head in ("all:", "gm_wall_mesh_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_mesh_test") for ln in lines if ln.startswith(head)] == [1], head
    assert sum("gm_wall_mesh_test.cpp" in ln and ln.startswith("\t$(CXX)") for ln in lines) == 1   # the rule's command


@pytest.mark.gpu
def test_host_wall_mesh_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_mesh_test ok" in r.stdout
