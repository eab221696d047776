"""GPU tests of the slots' streams (csrc/gm_api.hip create_slot_stream; DESIGN.md par. 7, "Frames in flight and hardware
queues"): the slots take their streams at the device's greatest priority, the /choppedCloud copy stream and the wall
map's stay at the default one.  Which hardware queue a stream lands on cannot be seen from here and is not asserted;
what is pinned is that nothing but timing changed: frames streamed over 4 and over 6 slots -- enqueued, replayed from
captured graphs, with a cloud output on every slot -- give the bytes of a one-slot context frame by frame, both values of
GM_STREAM_PRIORITY give the same bytes, and contexts opened and closed in a loop leave nothing behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

from geometric_mapping_amd import _lib, synth

pytestmark = pytest.mark.gpu
N = 30_000
RADIUS = synth.fixed_k_radius(N)
FLAGS = _lib.GM_CFG_DEFAULT | _lib.GM_CFG_RANSAC_CYLINDER | _lib.GM_CFG_KEEP_COUNTS
KW = dict(neighborRadius=RADIUS, max_points=N + 1, ransac_hypotheses=1024, ransac_threshold=0.03, ransac_seed=1)
MAX_SLOTS = 6            # more slots than any pool has queues by default
ISOLATED = np.array([[0.0, 3.6, 3.6]], dtype=np.float32)   # 5.09 m from the tunnel's axis: 3.09 m outside its wall, inside the crop box


def _frames():
    return [synth.tunnel_frame(N, seed=300 + i) for i in range(2 * MAX_SLOTS)]   # two rounds per slot of the widest context


def _outputs(c, slot, res):
    cloud, rows = c.cropped_cloud(slot)
    cen, cnt = c.voxel_centroids(slot)
    return dict(scatter6=res["scatter6"], eigenvectors=res["eigenvectors"],
                counts=np.array([res[k] for k in ("n_in", "n_cropped", "n_valid", "n_voxels")], dtype=np.int64),
                cylinder=res["cylinder"], cylinder_inliers=np.array([res["cylinder_inliers"]], dtype=np.int64),
                normals=c.normals(slot), cloud=cloud, rows=rows, voxel_centroids=cen, voxel_counts=cnt,
                neighbor_counts=c.neighbor_counts(slot))


def _stream(c, frames, slots, fetch=_outputs):
    """frames[i] on slot i % slots with `slots` frames in flight; every frame's outputs are fetched after its wait and
    before its slot is submitted to again."""
    out, inflight = [None] * len(frames), []
    for i, f in enumerate(frames):
        if len(inflight) == slots:
            j = inflight.pop(0)
            out[j] = fetch(c, j % slots, c.wait_frame(j % slots))
        c.submit_frame(i % slots, f)
        inflight.append(i)
    for j in inflight:
        out[j] = fetch(c, j % slots, c.wait_frame(j % slots))
    return out


def _same(got, ref):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (i, k)


@pytest.fixture(scope="module")
def frames():
    return _frames()


@pytest.fixture(scope="module")
def ref(gm, frames):
    """Every frame through a one-slot context, one at a time: what every other context has to reproduce."""
    with gm.GeometricMapping(flags=FLAGS, n_slots=1, **KW) as c:
        out = _stream(c, frames, 1)
    for f, o in zip(frames, out):   # (the tunnel is 12 m long, the crop box 10: five sixths of a frame are inside)
        inside = int(np.all(np.abs(f) <= 5.0, axis=1).sum())
        assert 0.8 * N < inside == o["counts"][1] == o["counts"][2]            # every cropped point keeps its normal
        assert o["cylinder_inliers"][0] > 0.5 * N and np.isfinite(o["normals"]).all()
    return out


@pytest.mark.parametrize("n_slots", [4, 6])
def test_frames_in_flight_equal_one_slot(gm, frames, ref, n_slots):
    with gm.GeometricMapping(flags=FLAGS, n_slots=n_slots, **KW) as c:
        _same(_stream(c, frames[:2 * n_slots], n_slots), ref[:2 * n_slots])


@pytest.mark.parametrize("n_slots", [1, 4, 6])
def test_graph_replay_on_slot_streams_equals_one_slot(gm, frames, ref, n_slots):
    """GM_CFG_GRAPH: capture and replay on the slots' streams.  Every slot sees two frames of one size from host rows: one
    capture per slot, replayed for the second round."""
    lib = _lib.load()
    with gm.GeometricMapping(flags=FLAGS | _lib.GM_CFG_GRAPH, n_slots=n_slots, **KW) as c:
        _same(_stream(c, frames[:2 * n_slots], n_slots), ref[:2 * n_slots])
        assert [lib.gm_debug_graph_captures(c._ctx, s) for s in range(n_slots)] == [1] * n_slots


def test_cloud_output_on_every_slot(gm, frames, ref):
    """/choppedCloud into a caller's buffer on every slot of a four-slot context: the copy stream (default priority) and
    the slot's stream (greatest priority) are ordered through events only.  Frame 3 has an isolated point appended and
    frame 6 the same point in the middle of its rows: the point loses its normal, so the rows from it on are sent again
    behind the compaction (k_rows_to_host).  The host rows [:n_valid] are those of cropped_cloud()."""
    fs = list(frames[:8])
    fs[3] = np.concatenate([fs[3], ISOLATED])
    fs[6] = np.concatenate([fs[6][:N // 2], ISOLATED, fs[6][N // 2:]])
    with gm.GeometricMapping(flags=FLAGS, n_slots=4, **KW) as c:
        bufs = [c.cloud_output_into(s, np.full((N + 1, 4), np.nan, dtype=np.float32)) for s in range(4)]

        def fetch(c, slot, res):
            o = _outputs(c, slot, res)
            n = res["n_valid"]
            assert n == len(o["cloud"]) > 0
            o["host_cloud"] = bufs[slot][:n, :3].copy()
            o["host_rows"] = bufs[slot][:n, 3].copy().view(np.int32)
            return o
        out = _stream(c, fs, 4, fetch)
    for i, o in enumerate(out):
        assert np.array_equal(o["host_cloud"], o["cloud"]) and np.array_equal(o["host_rows"], o["rows"]), i
        if i in (3, 6):
            at = N if i == 3 else N // 2
            keep = np.all(np.abs(fs[i]) <= 5.0, axis=1)
            assert keep[at] and o["counts"][1] == keep.sum() and o["counts"][2] == keep.sum() - 1   # cropped with the point, valid without it
            keep[at] = False
            assert np.array_equal(o["rows"], np.flatnonzero(keep)) and np.array_equal(o["cloud"], fs[i][keep])
            assert np.array_equal(o["counts"][1:3], ref[i]["counts"][1:3] + (1, 0))   # no other point lost its normal
    plain = [i for i in range(8) if i not in (3, 6)]
    _same([{k: v for k, v in out[i].items() if not k.startswith("host_")} for i in plain], [ref[i] for i in plain])


def _child(path):
    """(child process of test_stream_priority_values_agree: GM_STREAM_PRIORITY is read once per process)"""
    import geometric_mapping_amd as g
    with g.GeometricMapping(flags=FLAGS, n_slots=4, **KW) as c:
        out = _stream(c, _frames()[:8], 4)
    np.savez(path, **{f"{i}.{k}": v for i, o in enumerate(out) for k, v in o.items()})


def test_stream_priority_values_agree(gm, ref, tmp_path):
    """GM_STREAM_PRIORITY=default (the slots' streams as they used to be) and =high in a process each: the same bytes,
    and those of the one-slot context of this process."""
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    for value in ("default", "high"):
        path = str(tmp_path / f"{value}.npz")
        code = f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import test_gpu_slot_streams as t; t._child({path!r})"
        subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GM_STREAM_PRIORITY=value), check=True, timeout=120)
        with np.load(path) as z:
            got[value] = [{k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(f"{i}.")} for i in range(8)]
    _same(got["default"], got["high"])
    _same(got["high"], ref[:8])


def test_contexts_opened_and_closed_in_a_loop(gm, frames, ref):
    """32 four-slot contexts, one after the other (a stream or a hardware queue that is not given back would run out or
    fail well before that); every block is released, and the last context still computes its frames."""
    lib = _lib.load()
    first = lib.gm_debug_live_buffers()
    for k in range(32):
        with gm.GeometricMapping(flags=FLAGS, n_slots=4, **KW) as c:
            if k % 8 == 0:                               # (streams that have carried work are returned too)
                c.submit_frame(k % 4, frames[0])
                assert c.wait_frame(k % 4)["n_valid"] == ref[0]["counts"][2]
            if k == 31:
                _same(_stream(c, frames[:4], 4), ref[:4])
        assert lib.gm_debug_live_buffers() == first
