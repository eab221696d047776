"""tests/normals_np.py held against the C restatement and against itself, on the CPU, in every suite run:
  * the integer neighbour counts of the tie clouds equal the C oracle's, and FLANN's fp32 chain restated in numpy is exact
    on them (every pair with d2 < 4 M): the three references of the tie cases agree before a GPU is asked;
  * the plan twin's windows hold every neighbour: counting inside them gives the oracle's counts, on the usual grid and
    on the finer ones -- a twin whose windows, rows or tiles were wrong would lose neighbours here;
  * every case of the table reaches the mechanism it is listed for, and the table as a whole reaches every mechanism key:
    the coverage claims of tests/test_gpu_normals_edges.py, checkable without a GPU;
  * grid() reproduces two configurations worked out by hand.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_np as nn  # noqa: E402

TIE_CASES = [name for name, c in nn.CASES.items() if c.tie is not None]


def test_grid_of_the_1m_frame_and_of_the_clamp():
    # the 1 M-point bench frame ("k_normals"): bound 5, r = 0.5 sqrt(50 000 / 1e6) = 0.1118034, hr = 0.1119152,
    # 10 / hr = 89.35 -> 90 rows per axis; 90 * 90 * (90 * 64 + 64) = 4.7e7 < 2^31 -> x 64 times finer,
    # 640 / hr = 5718.6 -> 5719 cells; estimate 10 * 1 048 576 * 4.18879 r^3 / 1000 = 61 neighbours -> D = 1
    g = nn.grid(5.0, 0.5 * np.sqrt(50000.0 / 1e6), 1_000_000)
    assert (g["ns"], g["D"], g["ny"], g["nz"], g["fine"], g["nx"], g["xreach"], g["span"]) == (1 << 20, 1, 90, 90, 64, 5719, 65, 192)
    assert g["r2"] == np.float32(0.0125) and g["snap"] == 2.0 ** -21 and g["reach"][1, 1] == 65 and g["reach"][2, 0] == 0
    assert abs(float(g["band"]) / (2e-5 * 1.001 ** 2 * 0.0125) - 1.0) < 1e-6
    assert g["dscale"] == 2.0 ** 22 and 1.0 <= g["dband"] < 2.0             # 1 / band = 3.99e6 = 0.95 * 2^22
    # radius 0.001 in a +-20 box: the cell edge is clamped to ext / 1023 (1024 rows per axis at most), and 1024 * 1024 rows
    # leave 31 - 20 bits for x: fine = 1
    g = nn.grid(20.0, 0.001, 5000)
    assert g["hr"] == np.float32(40.0) / np.float32(1023.0) and (g["ny"], g["nz"], g["fine"], g["nx"], g["D"]) == (1024, 1024, 1, 1024, 1)
    assert g["r2"] == np.float32(1e-6)
    # D = 4 from an estimate of 2 000: r = 0.5 on the 1 M frame (5 489), per-row reaches shrink away from the tile's row
    g = nn.grid(5.0, 0.5, 1_000_000)
    assert g["D"] == 4 and g["ny"] == 80 and g["reach"][0, 0] == g["xreach"] == 65
    # four rows away: gap 3 h = 0.375375, sqrt(0.25 - 0.140906) * 64 / 0.5005 = 42.2 -> 42 + 2; diagonally: 2 * 0.140906 > r^2
    assert g["reach"][4, 0] == g["reach"][0, 4] == 44 and g["reach"][4, 4] == 0 and g["reach"][1, 1] == 65


@pytest.mark.parametrize("name", TIE_CASES)
def test_integer_counts_equal_the_oracle_on_tie_clouds(oc, name):
    xyz, radius = nn.case(name)
    q, up = nn.CASES[name].tie
    _, o_cnt = oc.normals(xyz, radius, oc.F64)
    assert np.array_equal(nn.tie_counts(q, up), o_cnt)
    if up:      # one ulp more of r2 turns exactly the ties into neighbours
        ties = nn.case_census(name)[0]
        assert int(nn.tie_counts(q, True).sum()) - int(nn.tie_counts(q, False).sum()) == ties > 0


@pytest.mark.parametrize("q", sorted(nn.TIE_M))
def test_flann_chain_is_exact_on_tie_clouds(q):
    P, u = nn.tie_points(q)
    # (the 2^-14 lattice: d2 beyond 2^24 steps has no fp32 of its own -- exact up to there, i.e. past the threshold)
    assert nn.flann_is_exact(P, u, nn.TIE_M[q], below=(1 << 24) + 1 if q in nn.PLANTED else None)
    if q == 10:
        assert nn.flann_is_exact(P, u * 1024, nn.TIE_M[q])


@pytest.mark.parametrize("name,rows", [("comb_p0", None), ("tunnel_n4095", None), ("row_q33", None), ("cluster_64", None),
                                       ("row_q33", 2), ("row_q33", 4), ("comb_p0", 4), ("tunnel_n4095", 3)])
def test_the_twins_windows_hold_every_neighbour(oc, name, rows):
    xyz, radius = nn.case(name)
    p, s = nn.case_plan(name, rows)
    assert s["D"] == (rows or 1)
    sx = xyz[p["order"]]
    _, o_cnt = oc.normals(xyz, radius, oc.F64)
    r2 = p["g"]["r2"]
    got = np.zeros(p["n"], np.int64)
    seen = np.zeros(p["n"], bool)
    for t in p["tiles"]:
        q = np.arange(t["s"], t["s"] + t["qn"])
        assert not seen[q].any() and 1 <= t["qn"] <= nn.TILE_Q
        seen[q] = True
        for gi in range(t["ngroups"]):
            qq = q[nn.GROUP_Q * gi:nn.GROUP_Q * (gi + 1)]
            for b, e in zip(t["wb"][:, gi], t["we"][:, gi]):
                if e > b:
                    got[qq] += (nn.flann_d2(sx[qq], sx[b:e]) < r2).sum(axis=1)
    assert seen.all()
    assert np.array_equal(got, o_cnt[p["order"]])


@pytest.mark.parametrize("name", list(nn.CASES))
def test_case_reaches_what_it_is_listed_for(name):
    c = nn.CASES[name]
    got = nn.reached(name)
    assert c.mech <= got, (name, sorted(c.mech - got))
    _, s = nn.case_plan(name)
    assert s["D"] == 1                                  # the frame path's own choice on every case
    assert (np.abs(nn.case(name)[0]) <= np.float32(c.bound)).all()
    if c.tie is not None:
        q, _ = c.tie
        ties, inb, near = nn.case_census(name)
        band_units = float(nn.case_plan(name)[0]["g"]["band"]) / (nn.tie_points(q)[1] * c.bound / 5.0) ** 2
        assert (ties >= 1000 and band_units < 1) if q == 7 else (inb >= 40 and band_units > 1)
        assert 400 < np.median(nn.tie_counts(q, False)) < 650
        if q in nn.PLANTED:                               # planted pairs: at the threshold and within two steps of it,
            assert ties >= 500 and nn.near_tie_pairs(q) - ties >= 2000 and band_units > 2   # all of them inside the band


@pytest.mark.parametrize("name,rows", nn.FINE_VARIANTS)
def test_fine_row_variants_reach_their_instantiation(name, rows):
    got = nn.reached(name, rows)
    assert {f"fine_D{rows}", "fine_pieces_4"} <= got and (rows != 4 or "fine_passes_3" in got)


def test_the_table_reaches_every_mechanism():
    got = set().union(*(nn.reached(name) for name in nn.CASES), *(nn.reached(n, d) for n, d in nn.FINE_VARIANTS))
    assert got >= set(nn.ALL_MECH), sorted(set(nn.ALL_MECH) - got)
    # the stream's edges, spelled out (a stream is whole octets: its total sits ON the chunk grid or whole octets away; the
    # +-1 edges are those of a row's last candidate)
    for key in ("stream_total_mod128_0", "row_end_mod128_0", "row_end_mod128_1", "row_end_mod128_127", "len_mod8_0",
                "len_mod8_1", "len_mod8_7", "empty_first", "empty_middle", "empty_last", "run_start_120", "chunks_1",
                "chunks_2", "chunks_4plus"):
        assert key in nn.ALL_MECH
