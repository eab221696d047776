"""The C++ host mirror's quantities (host/gm_wall_quantities_test.cpp, plain g++ over the C ABI):
Processor::wallMapQuantities against a direct gm_wall_map_quantities call and a scalar restatement of the rule, with zones,
two profiles and a baseline, and Processor::wallQuantityMetrics and wallQuantityRuns, which must name the planted
underbreak, pocket and lining."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_wall_quantities_test")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_wall_quantities_test"], check=True, capture_output=True)


def test_host_wall_quantities_builds_and_is_declared():
    _build()
    assert os.path.exists(EXE)
    hdr = open(os.path.join(ROOT, "host", "gm_tunnel_processing.hpp")).read()
    assert "gm_wall_quantities_info wallMapQuantities(unsigned station0, unsigned n, const std::vector<int32_t> &lo_q," in hdr
    assert "static struct gm_wall_quantity_metrics wallQuantityMetrics(const gm_wall_params &params, const gm_wall_quantity &record);" in hdr
    assert "static std::vector<gm_wall_quantity_run> wallQuantityRuns(const gm_wall_params &params," in hdr
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    lines = mk.splitlines()
    for head in ("all:", "gm_wall_quantities_test:", "\trm -f "):   # all, the rule, clean each know the binary, once
        assert [ln.replace(":", " ").split().count("gm_wall_quantities_test") for ln in lines if ln.startswith(head)] == [1], head
    assert sum("gm_wall_quantities_test.cpp" in ln and ln.startswith("\t$(CXX)") for ln in lines) == 1   # the rule's command
    assert "host/gm_wall_quantities_test" in open(os.path.join(ROOT, ".gitignore")).read().split()


@pytest.mark.gpu
def test_host_wall_quantities_on_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_wall_quantities_test ok" in r.stdout
