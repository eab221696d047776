"""One rule per design axis: an alignment's point, project and add plan on an arc or a clothoid element are the element
map's own gm_wall_arc_* / gm_wall_clothoid_* results, byte for byte.  Device-free calls of the C ABI alone: no GPU.

One- and two-element alignments of arcs (curvature 0.01, 0.02) and of clothoids (from 0.01 at +4e-4 / m, back from 0.02 at
-4e-4 / m), 100 stations each, on a tilted design direction away from the origin.  Per element 2000 seeded (chainage inside
the element, angle, rho in [1.8, 2.2]) triples -- 12 000 points, none left out -- and 50 seeded poses."""
import os
import subprocess

import numpy as np
import pytest

from geometric_mapping_amd import api

PRM = dict(t_min=3.0, station_length=0.25, radius=2.0, gate=0.25, direction=(0.9, 0.3, 0.1), point=(5.0, -3.0, 2.0))
TURN = (0.6, -0.8)
NST = 100


def _el(kind, curvature, rate=0.0):
    return dict(kind=kind, n_stations=NST, turn=TURN, curvature=curvature, rate=rate)


ALIGNMENTS = {
    "arc": [_el("arc", 0.01)],
    "arc_arc": [_el("arc", 0.01), _el("arc", 0.02)],
    "clothoid": [_el("clothoid", 0.01, 4e-4)],
    "clothoid_clothoid": [_el("clothoid", 0.01, 4e-4), _el("clothoid", 0.02, -4e-4)],
}


def _bits(*arrays):
    return np.concatenate([np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in arrays]).view(np.uint64)


def _element_rule(rule, i):
    """(params, axis struct, point, project, add_frame) of element i's own map"""
    p, arc, cl = rule.element_params(i)
    assert (arc is None) != (cl is None)
    if arc is not None:
        return p, arc, api.wall_arc_point, api.wall_arc_project, api.wall_arc_add_frame
    return p, cl, api.wall_clothoid_point, api.wall_clothoid_project, api.wall_clothoid_add_frame


def _span(p):
    return p.t_min, p.t_min + p.n_stations * p.station_length


@pytest.mark.parametrize("name", sorted(ALIGNMENTS))
def test_alignment_point_and_project_are_the_elements_own(name):
    rule = api.WallAlignmentRule(ALIGNMENTS[name], **PRM)
    assert rule.check() == 0
    for i in range(rule.n_elements):
        p, ax, point, project, _ = _element_rule(rule, i)
        rng = np.random.default_rng(1000 + 10 * sorted(ALIGNMENTS).index(name) + i)
        s0, s1 = _span(p)
        s = s0 + (s1 - s0) * rng.random(2000)
        s = np.minimum(s, np.nextafter(s1, s0))   # inside the element
        ph = 2.0 * np.pi * rng.random(2000)
        rho = 1.8 + 0.4 * rng.random(2000)
        own = point(p, ax, s, ph, rho)
        got = rule.point(s, ph, rho)
        assert np.array_equal(_bits(got), _bits(own))
        el, cs, ca, ce = rule.project(own)
        assert np.array_equal(el, np.full(2000, i))   # no point left out
        os_, oa, oe = project(p, ax, own)
        assert np.array_equal(_bits(cs, ca, ce), _bits(os_, oa, oe))


def test_axis_dump_builds_and_runs(tmp_path):
    """host/gm_wall_axis_dump.cpp, the program two builds of the host files are compared with: it builds from the two
    device-free files alone, accepts its accepted inputs and refuses its refused ones, and prints the same text twice."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "geometric_mapping_amd", "csrc")
    exe = str(tmp_path / "gm_wall_axis_dump")
    subprocess.run([os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"), "--offload-host-only", "-std=c++17", "-O1",
                    os.path.join(csrc, "gm_wall_host.hip"), os.path.join(csrc, "gm_wall_alignment_host.hip"),
                    os.path.join(root, "host", "gm_wall_axis_dump.cpp"), "-o", exe], check=True, capture_output=True)
    runs = [subprocess.run([exe], capture_output=True, text=True, timeout=120) for _ in range(2)]
    assert runs[0].returncode == 0 and runs[0].stdout == runs[1].stdout
    lines = runs[0].stdout.splitlines()
    assert len(lines) > 6000
    checks = [ln for ln in lines if " check st=" in ln]
    assert len(checks) == 12 and all(ln.endswith("st=0 ") for ln in checks)
    refusals = [ln for ln in lines if ln.startswith("refusal ")]
    assert len(refusals) > 50 and not any(ln.endswith("st=0") for ln in refusals)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0.0:
        q[:, 0] = -q[:, 0]
    return q


@pytest.mark.parametrize("name", sorted(ALIGNMENTS))
def test_add_plan_anchor_is_the_elements_own_add_frame(name):
    rule = api.WallAlignmentRule(ALIGNMENTS[name], **PRM)
    rules = [_element_rule(rule, i) for i in range(rule.n_elements)]
    for i, (p, ax, point, _, _) in enumerate(rules):
        rng = np.random.default_rng(2000 + 10 * sorted(ALIGNMENTS).index(name) + i)
        s0, s1 = _span(p)
        s = np.minimum(s0 + (s1 - s0) * rng.random(50), np.nextafter(s1, s0))
        tr = point(p, ax, s, 2.0 * np.pi * rng.random(50), 0.5 * rng.random(50))
        for k in range(50):
            pose = np.concatenate([_rotation(rng), tr[k].reshape(3, 1)], axis=1)
            plan = rule.add_plan(pose, 10.0)
            assert plan["element"] == i and i in plan["side_element"]
            for side, anchor in zip(plan["side_element"], plan["side_anchor"]):
                sp, sax, _, _, add_frame = rules[side]
                assert anchor == add_frame(sp, sax, pose)["anchor_station"]
