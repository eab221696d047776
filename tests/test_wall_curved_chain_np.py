"""CPU conditions of tests/test_gpu_wall_curved_chain.py, from the fp32 twins alone: every frame it uses leaves at least
0.999 of its points decidable, the guard clouds hold what each family needs, and its assertions tell a subtly wrong chain
from the right one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curved_chain_cases as cc  # noqa: E402
import fp32_np as fp  # noqa: E402
import wall_arc_np as wa  # noqa: E402
import wall_clothoid_np as wl  # noqa: E402
import wall_np as wn  # noqa: E402

F = np.float32


def _twin(c, gate=None, cloud=None, labels=None):
    return cc.twin(c, cc.reported_frame(c), c["cloud"] if cloud is None else cloud, c["labels"] if cloud is None else labels, gate)


@pytest.mark.parametrize("name", cc.NAMES)
def test_frames_are_decidable(name):
    """At least 0.999 of a frame's non-plane points are not uncertain, under the map's gate and the check's; every class
    occurs; the start is the one the frame's name says; the fp32 twin's classes are the fp64 twin's off both masks,
    where the fp64 twin computes the same thing."""
    c = cc.case(name)
    f = cc.reported_frame(c)
    if name.startswith("clothoid"):
        k = abs(float(f["kappa"]))
        assert (k == 0.0) if name.endswith("tangent_zero") else (0.0 < k < 1e-6) if name.endswith("tangent_tiny") else (k > 1e-3)
    for gate in (None, cc.CHECK_GATE):
        r = _twin(c, gate)
        counts = wa.class_counts(r)
        print(f"{name} gate {gate}: not uncertain {cc.share(r):.5f}, (mapped, outside, beyond_gate, plane) = {counts}")
        assert cc.share(r) >= 0.999
        assert counts[0] > 1000 and counts[2] > 30 and counts[3] > 300 and (counts[1] > 300 or name == "arc:ties")
        if "tangent" not in name:     # (26 m from a tangent start the device's two Newton steps do not converge; fp64's eight do)
            r64 = (wa if c["kind"] == "arc" else wl).points(c["cloud"], c["labels"], f, c["p"], gate=c["p"]["gate"] if gate is None else gate)
            off = ~r["uncertain"] & ~r64["ambiguous"]
            assert np.array_equal(r["cls"][off], r64["cls"][off]) and np.array_equal(r["cell"][off], r64["cell"][off])
        assert cc.assert_chain(c, r, r["e"], r["cell"], wa.class_counts(r, ~r["uncertain"])) == 0   # the twin passes its own pins


REQUIRED = {"arc": ("cy_in_gate", "big", "not_finite"),
            "clothoid:tangent": ("den", "g_in_gate", "phase", "big", "not_finite"),
            "clothoid:turned": ("cy_in_gate", "big", "not_finite")}


@pytest.mark.parametrize("name", cc.GUARD_NAMES)
def test_guard_clouds(name):
    """Every family has at least 32 points at which the twin says that its guard fires, none of them uncertain, all of
    them beyond_gate unless labelled plane.  The searches for guard points whose e ends within the gate found: cy <= 0 on
    both axes (the wall a quarter turn along the axis); a final |g| above the bound; a Newton denominator <= 0.25 with
    everything else quiet (the wall just past the end of the map, 24 of 30 000 draws).  No search was made for points of
    1e30, a phase of 2^20 or coordinates that are not finite that end within the gate: their e is NaN or infinite."""
    c = cc.guard_case(name)
    r = _twin(c)
    fam, live = c["family"], c["labels"] == 0
    assert not r["uncertain"].any() and not ("e_mixed" in r and r["e_mixed"].any())
    assert np.all(r["cls"][(fam >= 0) & live] == wn.BEYOND) and np.all(r["cell"][fam >= 0] == -1)
    assert (r["cls"][fam < 0] == wn.MAPPED).sum() > 1000
    gate = F(c["p"]["gate"])
    of = {k: (fam == i) & live for i, k in enumerate(c["names"])}
    for k in REQUIRED[name]:
        assert of[k].sum() >= cc.PER_FAMILY, (k, of[k].sum())
    in_gate = np.abs(r["e"]) <= gate
    if "cy_in_gate" in of:
        assert np.all(r["cy"][of["cy_in_gate"]] < 0.0) and np.all(in_gate[of["cy_in_gate"]])
    if name == "arc":
        assert np.all(r["cy"][of["cy_past_centre"]] < 0.0) and of["cy_past_centre"].sum() >= 8
    if name == "clothoid:tangent":
        assert r["tangent"] and np.all(r["cy"][np.isfinite(c["cloud"]).all(axis=1)] == 1.0)
        low = ~(r["dens"] > F(0.25))
        assert np.all(low.any(axis=0)[of["den"] | of["den_in_gate"]])
        assert low[0][of["den"]].sum() >= 8 and (low[1] & ~low[0])[of["den"]].sum() >= 8       # the first and the second step
        big_g = np.abs(r["g"]) > F(wl.G_BOUND)
        assert np.all((big_g & in_gate & ~low.any(axis=0))[of["g_in_gate"]])
        assert of["den_in_gate"].sum() >= 8 and np.all((in_gate & ~big_g & np.isfinite(r["t"]))[of["den_in_gate"]])
        assert np.all(np.isnan(r["g"][of["phase"]])) and np.all(np.isfinite(c["cloud"][of["phase"]]))
    if name == "clothoid:turned":
        quiet = np.all(r["dens"] > F(0.25), axis=0) & (np.abs(r["g"]) <= F(wl.G_BOUND))
        assert np.all(quiet[of["cy_in_gate"]])
    assert not np.isfinite(r["e"][of["big"]]).any() or name == "arc"
    assert np.all(~np.isfinite(r["e"][of["big"]]) | ~np.isfinite(r["t"][of["big"]]))
    assert np.all(np.isnan(r["e"][of["not_finite"]]))
    counts = wa.class_counts(r)
    assert cc.assert_guards(c, r, r["e"], r["cell"], counts) == 0


@pytest.mark.parametrize("kind", ["arc", "clothoid"])
def test_far_station_clouds(kind):
    """Both sides of wall_station's |jl| < 4e18: every point is within the gate and outside, 32 of them merely so."""
    c = cc.far_station_case(kind)
    f = cc.reported_frame(c)
    r = _twin(c, cloud=c["cloud"])
    assert not f["o"].any() and abs(int(f["anchor_station"])) < 10 ** 6
    assert np.all(r["cls"] == wn.OUTSIDE) and not r["uncertain"].any() and np.all(np.abs(r["e"]) <= F(c["p"]["gate"]))
    far = np.abs(r["jl"]) >= F(4.0e18)
    assert far.sum() == 48 and (~far).sum() == 32 and np.abs(r["jl"][~far]).min() > 1e17 and np.abs(r["jl"][far]).max() < 3e20


def _device_of(r):
    return r["e"], r["cell"], wa.class_counts(r, ~r["uncertain"])


def _fails(assertion, *a):
    with pytest.raises(AssertionError):
        assertion(*a)


def test_the_pins_see_a_subtly_wrong_chain(monkeypatch):
    """Chains that are wrong the way a kernel could be, each run as if it were the device against the right twin: the
    assertions of the GPU file fail on every one of them."""
    arc, tangent = cc.case("arc:ties"), cc.case("clothoid:tangent_zero")
    osc = cc.case("clothoid:oblique_s")
    g_arc, g_tan, g_turn = (cc.guard_case(k) for k in cc.GUARD_NAMES)
    right = {id(c): _twin(c) for c in (arc, tangent, osc, g_arc, g_tan, g_turn)}

    def wrong(c):
        return _device_of(_twin(c))

    # the last bit of one coefficient of the sine's or the cosine's polynomial.  (Of the six, these three: the last bit of
    # the two highest of the cosine and the highest of the sine moves a value by 1e-4 of its own last bit at these phases,
    # which 4097 points do not resolve.)
    for name, i in (("SIN_C", 1), ("SIN_C", 2), ("COS_C", 2)):
        with monkeypatch.context() as mp:
            coef = getattr(wl, name).copy()
            coef[i] = fp.ulp_steps(coef[i], 1)
            mp.setattr(wl, name, coef)
            _fails(cc.assert_chain, tangent, right[id(tangent)], *wrong(tangent))
    # the third term of the reduction by pi / 2 dropped
    with monkeypatch.context() as mp:
        mp.setattr(wl, "PIO2", np.array([wl.PIO2[0], wl.PIO2[1], 0.0], F))
        _fails(cc.assert_chain, tangent, right[id(tangent)], *wrong(tangent))
    # the weights of the first two nodes swapped (the second and the third are equal: swapping those is no defect)
    with monkeypatch.context() as mp:
        mp.setattr(wl, "GL4_W", wl.GL4_W[[1, 0, 2, 3]])
        _fails(cc.assert_chain, tangent, right[id(tangent)], *wrong(tangent))
        _fails(cc.assert_chain, osc, right[id(osc)], *wrong(osc))
    # the den > 0.25 test removed: the denominator points that end within the gate become outside
    with monkeypatch.context() as mp:
        mp.setattr(wl, "GUARD_DEN", False)
        _fails(cc.assert_guards, g_tan, right[id(g_tan)], *wrong(g_tan))
    # the cy > 0 test removed, on both axes
    with monkeypatch.context() as mp:
        mp.setattr(wa, "GUARD_CY", False)
        _fails(cc.assert_guards, g_arc, right[id(g_arc)], *wrong(g_arc))
        _fails(cc.assert_guards, g_turn, right[id(g_turn)], *wrong(g_turn))
    # the fma the twins had: the sum in fp64, rounded again
    with monkeypatch.context() as mp:
        mp.setattr(wa, "fma", fp.fma32_double_rounding)
        _fails(cc.assert_chain, arc, right[id(arc)], *wrong(arc))
    for c in (arc, tangent, osc):                      # and the right chain passes
        assert cc.assert_chain(c, right[id(c)], *wrong(c)) == 0
